"""GPU: the difference string rendered on the device from bytes (include/wfa_hip.h: wfahip_diff_text_device; Aligner.diff_tensors).
The kernels on the synthetic records, ops and sequences of tests/diff_cases.py -- every byte value, the trim cases with windows only
the record can name, ops that render nothing, the seams of the 64-op rounds, of the lane-per-op bound (gaps of 15, 16 and 17 letters)
and of the scan blocks, X runs across every residue of a 4-byte group, ops of 70 001 columns of every kind, a match run of ten digits
-- against the Python restatement and the host entry, byte for byte, at every shift of the text off a 4-byte boundary, with
everything behind the text still poisoned and the inputs unchanged; the capacity and validation errors, each next to the same
record at the bound; an empty batch; a caller-owned stream.  No test hands the write kernel anything the length kernel has not
accepted."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import altext_cases as A  # noqa: E402
import cigar_cases as K  # noqa: E402
import diff_cases as D  # noqa: E402
import diff_device as V  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al(built):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=True), device=0)
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def _cases():
    return D.cases()


@pytest.mark.parametrize("n", [1, 3, 4, 5, V.SCAN_BLOCK_PAIRS + 1])
@pytest.mark.parametrize("only", [0, 1])
def test_synthetic_records(al, only, n):
    picked = V.pick(_cases(), n)
    want = D.expected(picked, only)
    total = len(want[0])
    assert total > 0
    ins = V.render_and_compare(al, A.arrays(picked, seed=100 + n), picked, only)
    # out=None: one sizing call, then exactly the text
    text, off = al.diff_tensors(*ins, only_aligned=bool(only))
    assert text.numel() == total
    V.same_text(text, want[0], total)
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])


@pytest.mark.parametrize("n_ops", [64, 65, 129, 200])
def test_round_seams(al, n_ops):
    """op lists that end at, and one, 65 and 72 ops behind, a round of 64: the carry of bytes and bases between rounds"""
    cases = [c for c in _cases() if len(c[1] or []) == n_ops]
    assert cases
    for only in (0, 1):
        V.render_and_compare(al, A.arrays(cases, seed=n_ops), cases, only, shifts=(0, 3))


def test_lane_bound_seams_long_ops_and_every_byte_value(al):
    """diff_cases.extra_cases: gaps of 15, 16 and 17 letters and X runs of 5 and 6 columns -- the last an op's own lane renders and
    the first the wave sweeps --, X tokens across every residue of a group, one op of 70 001 columns of each kind, all 256 byte values"""
    cases = D.extra_cases() + [c for c in A.cases() if A.consumed(c[1] or [])[0] >= 70000]
    for only in (0, 1):
        V.render_and_compare(al, A.arrays(cases, seed=5), cases, only)


def test_ten_digit_match_run(al):
    """an M op of 1 000 000 007 columns: ten digits and not a base read; query and target are one zero-filled gigabyte"""
    import torch
    ops, n, whole = D.ten_digit_case(b"\0", b"\0")
    win = [np.array([v], np.int32) for v in (3, n - 3, 3, n - 3)]
    rec = V.dev(A.records(np.zeros(1, np.int32), np.zeros(1, np.uint64), np.array([3], np.uint32), win))
    blob = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    off0, len1 = V.dev(np.zeros(1, np.uint64)), V.dev(np.array([n], np.uint32))
    for only, want in ((False, whole), (True, b":%d" % D.TEN_DIGITS)):
        text, off = al.diff_tensors(rec, V.dev(np.array(ops, np.uint64)), blob, off0, len1, off0, len1, only_aligned=only)
        assert text.cpu().numpy().tobytes() == want and off.cpu().numpy().tolist() == [0, len(want)]
    del blob
    torch.cuda.empty_cache()


def test_capacity_errors_sizing_call_and_empty_batch(al):
    import torch
    from wfa_amd import _lib
    n = 5
    picked = V.pick(_cases(), n)
    want = D.expected(picked, 0)
    ins = V.inputs(A.arrays(picked, seed=100 + n))
    total = len(want[0])
    text = V.text_buf(total + 64)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    rc, need = V.raw(al, ins, 0, text, total - 1, off)                             # one below the total
    assert rc == _lib.ERR_OOM and need == total
    assert V.untouched(text)                                                       # the text untouched
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])              # d_text_off filled
    rc, need = V.raw(al, ins, 0, text, total, off)                                 # exactly the total: fits
    assert rc == 0 and need == total
    V.same_text(text, want[0], total)
    off.fill_(-1)
    rc, need = V.raw(al, ins, 0, None, 0, off)                                     # the sizing call
    assert rc == _lib.ERR_OOM and need == total and np.array_equal(off.cpu().numpy().view(np.uint64), want[1])
    with pytest.raises(_lib.WfaHipError) as ei:                                    # the wrapper: ERR_OOM with off filled
        al.diff_tensors(*ins, out=(text[:total - 1], off))
    assert ei.value.code == _lib.ERR_OOM and int(off[n]) == total
    # no pairs: d_text_off[0] = 0 and nothing else
    off.fill_(-1)
    text = V.text_buf(64)
    rc, need = V.raw(al, [ins[0][:0]] + ins[1:], 0, text, 64, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0] + [-1] * n
    assert V.untouched(text)
    t0, o0 = al.diff_tensors(ins[0][:0], ins[1], ins[2], *[t[:0] for t in ins[3:]])
    assert t0.numel() == 0 and o0.cpu().numpy().tolist() == [0]


# (only_aligned, what is wrong, the same thing at the bound): changes to altext_cases.PAIR -- 7 query bytes, 9 target bytes, trimmed
# 4M over query bytes [1, 5) and target bytes [2, 6)
CHECKS = [
    (0, dict(q_len=6), dict(q_len=7)),                      # the ops consume one query byte more than there is
    (0, dict(t_len=8), dict(t_len=9)),                      # ... one target byte
    (1, dict(qend=4), dict(qend=5)),                        # ... than the trimmed window holds
    (1, dict(tbegin=4), dict(tbegin=3)),
    (1, dict(qbegin=0), dict(qbegin=1)),                    # QBEGIN = 0
    (1, dict(tbegin=0, tend=3), dict(tbegin=1, tend=4)),
    (1, dict(qend=8), dict(qbegin=4, qend=7)),              # QEND = q_len + 1
    (1, dict(tend=10), dict(tbegin=6, tend=9)),
    (1, dict(qbegin=6, qend=4), dict(qbegin=2, qend=5)),    # QBEGIN - 1 > QEND
]
SIZES = [15, 2]   # the bytes of PAIR's string: +q-tt:4*zx+y-uv, and trimmed :4


@pytest.mark.parametrize("only,wrong,right", CHECKS)
def test_checks_of_the_length_kernel(al, only, wrong, right):
    import torch
    from wfa_amd import _lib
    text = V.text_buf(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    rc, _need = V.raw(al, V.inputs(A.one(**wrong)), only, text, 256, off)
    assert rc == _lib.ERR_BAD_ARG and V.untouched(text)
    rc, need = V.raw(al, V.inputs(A.one(**right)), only, text, 256, off)
    assert rc == 0 and need == SIZES[only]


@pytest.mark.parametrize("only", [0, 1])
def test_bytes_or_ops_outside_their_buffers(al, only):
    import torch
    from wfa_amd import _lib
    a = A.one()
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    ins = V.inputs(a)
    text = V.text_buf(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    end = int(max(q_off[0] + q_len[0], t_off[0] + t_len[0]))     # the later sequence of the pair ends there
    ops_end = int(a["ops_off"][0] + a["ops_len"][0])
    for kw in (dict(size=end - 1), dict(ops_cap=ops_end - 1), dict(size=0)):
        rc, _need = V.raw(al, ins, only, text, 256, off, **kw)
        assert rc == _lib.ERR_BAD_ARG and V.untouched(text), kw
    last = "q_off" if q_off[0] > t_off[0] else "t_off"
    last_len = int((q_len if last == "q_off" else t_len)[0])
    for v in (len(blob) - last_len + 1, len(blob), 1 << 63, (1 << 64) - 1):
        rc, _need = V.raw(al, V.inputs(A.one(**{last: v})), only, text, 256, off)
        assert rc == _lib.ERR_BAD_ARG and V.untouched(text), v
    # the same offsets on a pair that is not OK are never looked at: nothing renders, nothing is refused
    b = A.one(**{last: 1 << 63})
    b["status"][0] = K.NO_MEMORY
    rc, need = V.raw(al, V.inputs(b), only, text, 256, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0, 0, 0] and V.untouched(text)
    rc, need = V.raw(al, ins, only, text, 256, off, size=end, ops_cap=ops_end)   # both end exactly at their bounds
    assert rc == 0 and need == SIZES[only]
    got = text.cpu().numpy()
    assert got[:need].tobytes() == D.diff_of(A.PAIR, only) and (got[need:] == V.POISON).all()


def test_caller_owned_stream(al):
    import torch
    n = V.SCAN_BLOCK_PAIRS + 1
    picked = V.pick(_cases(), n)
    want = D.expected(picked, 1)
    ins = V.inputs(A.arrays(picked, seed=100 + n))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        text, off = al.diff_tensors(*ins, only_aligned=True, stream=s)
    V.same_text(text, want[0], len(want[0]))
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])
