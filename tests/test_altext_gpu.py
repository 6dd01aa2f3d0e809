"""GPU: the display rows rendered on the device (include/wfa_hip.h: wfahip_alignment_text_device; Aligner.alignment_text_tensors).
The kernels on synthetic records, ops and sequences (tests/altext_cases.py: every byte value, the trim cases with windows only the
record can name, ops without columns, the seams of the 64-op rounds, of the 4-column groups and the 256-column sweeps and of the
scan blocks, rows starting at every byte alignment) against AlignmentResult.AlignmentText, byte for byte, with everything behind
the rows still poisoned and the inputs unchanged; the capacity and validation errors, each next to the same record at the bound;
a caller-owned stream; and end to end over the oracle's alignments.  No test hands the write kernel anything the length kernel
has not accepted."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import altext_cases as A  # noqa: E402
import cigar_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
PAD = 64      # bytes behind the sequences in a blob that is ALIGNED on the device (the alignment kernels' loads at its tail)
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


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


def _inputs(a):
    """A.arrays' dict as the seven device tensors of the entry: rec, ops, blob, q_off, q_len, t_off, t_len"""
    rec = A.records(a["status"], a["ops_off"], a["ops_len"], a["win"])
    return [_dev(rec), _dev(a["ops"])] + [_dev(x) for x in a["seqs"]]


@functools.lru_cache(maxsize=None)
def _synthetic(n):
    """n cases -- the multi-round, moved-window and long-op pairs first, so that the smallest batches hold them; past the set the
    pairs of up to 1 025 columns repeat -- as host arrays, with both expected results"""
    cases = A.cases()
    ops_n = lambda c: len(c[1] or [])
    first = [c for c in cases if ops_n(c) == 200][:1] + [c for c in cases if A.consumed(c[1] or [])[0] > 5000]
    first += [c for c in cases if ops_n(c) in (65, 129)]
    pool = first + [c for c in cases if not any(c is f for f in first)]
    small = [c for c in pool if A.consumed(c[1] or [])[0] <= 1025]
    picked = pool[:n] + [small[i % len(small)] for i in range(max(0, n - len(pool)))]
    return A.arrays(picked, seed=100 + n), A.expected(picked, 0), A.expected(picked, 1)


def _raw(al, ins, only, planes, row_cap, off, stream=None, ops_cap=None, blob_bytes=None):
    """the C entry itself: (return code, *row_needed)"""
    import torch
    from wfa_amd import _lib
    torch.cuda.synchronize()  # (the fills of the test ran on torch's stream; stream=None is the context's own)
    rec, ops, blob, q_off, q_len, t_off, t_len = ins
    need = C.c_uint64(12345)
    ptrs = [p.data_ptr() if p is not None else None for p in planes]
    rc = _lib.lib().wfahip_alignment_text_device(al._ctx, rec.data_ptr(), ops.data_ptr(), ops.numel() if ops_cap is None else ops_cap,
                                                 blob.data_ptr(), blob.numel() if blob_bytes is None else blob_bytes, q_off.data_ptr(),
                                                 q_len.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), rec.shape[0], only, *ptrs,
                                                 row_cap, off.data_ptr(), C.byref(need), stream)
    return rc, need.value


def _planes(size, shift=0):
    """three poisoned planes of `size` bytes, `shift` bytes off a 4-byte boundary"""
    import torch
    return [torch.full((size + 4,), POISON, dtype=torch.uint8, device="cuda:0")[shift:shift + size] for _ in range(3)]


def _same_rows(got, want, total):
    for name, g, w in zip(("q_row", "a_row", "t_row"), got, want):
        g = g.cpu().numpy()
        bad = np.flatnonzero(g[:total] != w)
        assert bad.size == 0, f"{name}: first differing byte {bad[:1]} of {total}"
        assert (g[total:] == POISON).all(), name                  # nothing at or beyond d_row_off[n] is written


@pytest.mark.parametrize("n", [1, 3, 4, 5, SCAN_BLOCK_PAIRS + 1])
@pytest.mark.parametrize("only", [0, 1])
def test_synthetic_records(al, only, n):
    import torch
    a, *want = _synthetic(n)
    want = want[only]
    ins = _inputs(a)
    before = [t.clone() for t in ins]
    total = len(want[0])
    assert total > 0
    planes = _planes(total + 257)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    out = al.alignment_text_tensors(*ins, only_aligned=bool(only), out=(*planes, off))
    assert all(x is y for x, y in zip(out, (*planes, off)))
    got_off = off.cpu().numpy().view(np.uint64)
    assert got_off[0] == 0 and got_off[n] == total
    assert np.array_equal(got_off, want[3])
    _same_rows(planes, want, total)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))     # the inputs are only read
    # out=None: one sizing call, then exactly the rows
    q_row, a_row, t_row, o3 = al.alignment_text_tensors(*ins, only_aligned=bool(only))
    assert q_row.numel() == a_row.numel() == t_row.numel() == total
    _same_rows((q_row, a_row, t_row), want, total)
    assert np.array_equal(o3.cpu().numpy().view(np.uint64), want[3])


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_planes_off_a_4_byte_boundary(al, shift):
    """the byte-store path of the write kernel: the same rows"""
    import torch
    n = 5
    a, want, _ = _synthetic(n)
    total = len(want[0])
    planes = _planes(total + 61, shift)
    assert all(p.data_ptr() % 4 == shift for p in planes)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    al.alignment_text_tensors(*_inputs(a), out=(*planes, off))
    _same_rows(planes, want, total)
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[3])


def test_device_rows_equal_the_host_renderers(al):
    import wfa_amd
    n = 40
    a, _, _ = _synthetic(n)
    z = np.zeros(n, np.uint32)
    qbegin, qend, tbegin, tend = a["win"]
    br = wfa_amd.BatchResult(a["status"], z, tbegin, tend, qbegin, qend, z, z, z, z, a["ops_off"], a["ops_len"], a["ops"])
    for only in (False, True):
        host = wfa_amd.alignment_text(br, *a["seqs"], only_aligned=only, n_threads=3)
        dev = al.alignment_text_tensors(*_inputs(a), only_aligned=only)
        for h, d in zip(host, dev):
            assert np.array_equal(h.view(np.uint8), d.cpu().numpy().view(np.uint8))


def test_capacity_errors_and_sizing_call(al):
    import torch
    from wfa_amd import _lib
    n = 5
    a, want, _ = _synthetic(n)
    ins = _inputs(a)
    total = len(want[0])
    planes = _planes(total + 64)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    rc, need = _raw(al, ins, 0, planes, total - 1, off)
    assert rc == _lib.ERR_OOM and need == total
    assert all((p.cpu().numpy() == POISON).all() for p in planes)                  # the planes untouched
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[3])              # d_row_off filled
    rc, need = _raw(al, ins, 0, planes, total, off)                                # exactly the total: fits
    assert rc == 0 and need == total
    _same_rows(planes, want, total)
    off.fill_(-1)
    rc, need = _raw(al, ins, 0, [None] * 3, 0, off)                                # the sizing call
    assert rc == _lib.ERR_OOM and need == total and np.array_equal(off.cpu().numpy().view(np.uint64), want[3])
    # no pairs: d_row_off[0] = 0 and nothing else
    off.fill_(-1)
    planes = _planes(64)
    rc, need = _raw(al, [ins[0][:0]] + ins[1:], 0, planes, 64, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0] + [-1] * n
    assert all((p.cpu().numpy() == POISON).all() for p in planes)


# (only_aligned, what is wrong, the same thing at the bound): changes to altext_cases.PAIR -- 7 query bytes, 9 target bytes,
# trimmed 4M over query bytes [1, 5) and target bytes [2, 6)
CHECKS = [
    (0, dict(q_len=6), dict(q_len=7)),                      # the ops consume one query base more than there is
    (0, dict(t_len=8), dict(t_len=9)),                      # ... one target base
    (1, dict(qend=4), dict(qend=5)),                        # ... than the trimmed window holds
    (1, dict(tbegin=4), dict(tbegin=3)),
    (1, dict(qbegin=0), dict(qbegin=1)),                    # QBEGIN = 0
    (1, dict(tbegin=0, tend=3), dict(tbegin=1, tend=4)),
    (1, dict(qend=8), dict(qbegin=4, qend=7)),              # QEND = q_len + 1
    (1, dict(tend=10), dict(tbegin=6, tend=9)),
    (1, dict(qbegin=6, qend=4), dict(qbegin=2, qend=5)),    # QBEGIN - 1 > QEND
]


@pytest.mark.parametrize("only,wrong,right", CHECKS)
def test_checks_of_the_length_kernel(al, only, wrong, right):
    import torch
    from wfa_amd import _lib
    planes = _planes(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    rc, _need = _raw(al, _inputs(A.one(**wrong)), only, planes, 256, off)
    assert rc == _lib.ERR_BAD_ARG
    assert all((p.cpu().numpy() == POISON).all() for p in planes)
    rc, need = _raw(al, _inputs(A.one(**right)), only, planes, 256, off)
    assert rc == 0 and need == [11, 4][only]


@pytest.mark.parametrize("only", [0, 1])
def test_sequence_or_ops_outside_their_buffers(al, only):
    import torch
    from wfa_amd import _lib
    a = A.one()
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    ins = _inputs(a)
    planes = _planes(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    end = int(max(q_off[0] + q_len[0], t_off[0] + t_len[0]))
    ops_end = int(a["ops_off"][0] + a["ops_len"][0])
    for kw in (dict(blob_bytes=end - 1), dict(ops_cap=ops_end - 1), dict(blob_bytes=0)):
        rc, _need = _raw(al, ins, only, planes, 256, off, **kw)
        assert rc == _lib.ERR_BAD_ARG, kw
        assert all((p.cpu().numpy() == POISON).all() for p in planes)
    rc, need = _raw(al, ins, only, planes, 256, off, blob_bytes=end, ops_cap=ops_end)   # both end exactly at their bounds
    assert rc == 0 and need == [11, 4][only]
    last = "q_off" if q_off[0] > t_off[0] else "t_off"
    for v in (1 << 63, (1 << 64) - 1, len(blob)):
        rc, _need = _raw(al, _inputs(A.one(**{last: v})), only, planes, 256, off)
        assert rc == _lib.ERR_BAD_ARG, v
    got = [p.cpu().numpy() for p in planes]
    assert [g[:need].tobytes() for g in got] == list(A.rows_of(A.PAIR, only)) and all((g[need:] == POISON).all() for g in got)


def test_caller_owned_stream(al):
    import torch
    n = SCAN_BLOCK_PAIRS + 1
    a, _, want = _synthetic(n)
    ins = _inputs(a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        q_row, a_row, t_row, off = al.alignment_text_tensors(*ins, only_aligned=True, stream=s)
    _same_rows((q_row, a_row, t_row), want, len(want[0]))
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[3])


def _seqs(arrays):
    blob, q_off, q_len, t_off, t_len = arrays
    b = blob.tobytes()
    return ([b[int(o):int(o) + int(n)] for o, n in zip(q_off, q_len)], [b[int(o):int(o) + int(n)] for o, n in zip(t_off, t_len)])


@functools.lru_cache(maxsize=None)
def _batch(glob):
    """about 300 pairs, the oracle's results and AlignmentText of each, both modes.  Global: 150 bases @2 %, an empty pair, a pair
    with an N, A against C.  Semi-global: 300 bases @5 % with the target overhanging on both sides."""
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
    cases = [(int(w.status[i]), [int(x) for x in w.pair_ops(i)] if w.status[i] == 0 else None, qs[i], ts[i], int(w.qbegin[i]),
              int(w.qend[i]), int(w.tbegin[i]), int(w.tend[i])) for i in range(len(qs))]
    return arrays, w, [A.rows_of(c, 0) for c in cases], [A.rows_of(c, 1) for c in cases]


def _to_device(arrays):
    blob, q_off, q_len, t_off, t_len = arrays
    return (_dev(np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(PAD, np.uint8)])), _dev(np.asarray(q_off, np.uint64)), _dev(np.asarray(q_len, np.uint32)),
            _dev(np.asarray(t_off, np.uint64)), _dev(np.asarray(t_len, np.uint32)))


def _rows(q_row, a_row, t_row, off):
    planes, o = [p.cpu().numpy().tobytes() for p in (q_row, a_row, t_row)], off.cpu().numpy()
    return [tuple(p[int(o[i]):int(o[i + 1])] for p in planes) for i in range(len(o) - 1)]


@pytest.mark.parametrize("glob", [True, False])
def test_end_to_end_against_the_oracle(al, al_semi, glob):
    a = al if glob else al_semi
    arrays, w, full, trimmed = _batch(glob)
    dev = _to_device(arrays)
    rec, ops = a.align_tensors(*dev)
    assert np.array_equal(rec.cpu().numpy()[:, 0], w.status)
    assert _rows(*a.alignment_text_tensors(rec, ops, *dev)) == full
    assert _rows(*a.alignment_text_tensors(rec, ops, *dev, only_aligned=True)) == trimmed
    if glob:
        assert full[-3] == (b"", b"", b"") and full[-1] == (b"A", b" ", b"C") and trimmed[-1] == (b"", b"", b"")
        assert full[-2][1] == b"||||" + b" " + b"|" * 8
    else:
        assert sum(len(f[0]) != len(t[0]) for f, t in zip(full, trimmed)) > 100  # the overhangs are trimmed away


def test_bounded_records_render_empty(al):
    arrays, w, full, trimmed = _batch(True)
    bound = int(np.median(w.score[w.status == 0]))
    dev = _to_device(arrays)
    rec, ops = al.align_tensors(*dev, max_score=bound)
    st = rec.cpu().numpy()[:, 0]
    over = (w.status == 0) & (w.score > bound)
    assert over.sum() > 20 and (~over).sum() > 20
    assert (st[over] == 8).all() and np.array_equal(st[~over], w.status[~over])
    empty = (b"", b"", b"")
    assert _rows(*al.alignment_text_tensors(rec, ops, *dev)) == [empty if o else f for o, f in zip(over, full)]
    assert _rows(*al.alignment_text_tensors(rec, ops, *dev, only_aligned=True)) == [empty if o else t for o, t in zip(over, trimmed)]
