"""What tests/test_diff_gpu.py and tests/test_diff_packed_gpu.py share: the arrays of tests/altext_cases.py (bytes) or
tests/altext_pk_cases.py (words) as device tensors, the C entries themselves, a poisoned text buffer at any shift off a 4-byte
boundary, and the comparison against the restatement of tests/diff_cases.py and against the host entries.  An arrays dict with a "pk"
entry goes to the packed entries, one with "seqs" to the byte entries."""
import ctypes as C

import numpy as np

import altext_cases as A
import diff_cases as D

POISON = 0xA5
SCAN_BLOCK_PAIRS = 4096  # wfa_cigar.hip: CIG_SCAN_BLOCK * CIG_SCAN_ITEMS


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


def inputs(a):
    """the device tensors of an entry: rec, ops, then blob, q_off, q_len, t_off, t_len -- or words, q_woff, q_len, t_woff, t_len, q_rc"""
    rec = A.records(a["status"], a["ops_off"], a["ops_len"], a["win"])
    return [dev(rec), dev(a["ops"])] + [dev(x) for x in a["pk" if "pk" in a else "seqs"]]


def raw(al, ins, only, text, text_cap, off, stream=None, ops_cap=None, size=None):
    """the C entry itself -- the packed one for eight tensors, the byte one for seven: (return code, *text_needed)"""
    import torch
    from wfa_amd import _lib
    torch.cuda.synchronize()  # (the fills of the test ran on torch's stream; stream=None is the context's own)
    rec, ops, seqs = ins[:3]
    need = C.c_uint64(12345)
    head = [al._ctx, rec.data_ptr(), ops.data_ptr(), ops.numel() if ops_cap is None else ops_cap, seqs.data_ptr(),
            seqs.numel() if size is None else size] + [t.data_ptr() for t in ins[3:7]]
    tail = [rec.shape[0], only, text.data_ptr() if text is not None else None, text_cap, off.data_ptr(), C.byref(need), stream]
    if len(ins) == 8:
        rc = _lib.lib().wfahip_diff_text_packed_device(*head, ins[7].data_ptr() if ins[7] is not None else None, *tail)
    else:
        rc = _lib.lib().wfahip_diff_text_device(*head, *tail)
    return rc, need.value


def tensors(al, ins, **kw):
    """Aligner.diff_tensors or diff_tensors_packed on the tensors of inputs()"""
    if len(ins) == 8:
        return al.diff_tensors_packed(*ins[:7], q_rc=ins[7], **kw)
    return al.diff_tensors(*ins, **kw)


def host(a, only, n_threads=3):
    """the host entry on the same arrays: (text, off)"""
    import wfa_amd
    z = np.zeros(len(a["status"]), np.uint32)
    qbegin, qend, tbegin, tend = a["win"]
    br = wfa_amd.BatchResult(a["status"], z, tbegin, tend, qbegin, qend, z, z, z, z, a["ops_off"], a["ops_len"], a["ops"])
    if "pk" in a:
        return wfa_amd.diff_text_packed(br, *a["pk"], only_aligned=bool(only), n_threads=n_threads)
    return wfa_amd.diff_text(br, *a["seqs"], only_aligned=bool(only), n_threads=n_threads)


def text_buf(size, shift=0):
    """a poisoned buffer of `size` bytes, `shift` bytes off a 4-byte boundary"""
    import torch
    t = torch.full((size + 4,), POISON, dtype=torch.uint8, device="cuda:0")[shift:shift + size]
    assert t.data_ptr() % 4 == shift
    return t


def untouched(text):
    return bool((text.cpu().numpy() == POISON).all())


def same_text(got, want, total):
    g = got.cpu().numpy()
    bad = np.flatnonzero(g[:total] != want)
    assert bad.size == 0, f"first differing byte {bad[:1]} of {total}: got {g[:total].tobytes()[max(0, int(bad[0]) - 20):int(bad[0]) + 20]!r}"
    assert (g[total:] == POISON).all()                           # nothing at or beyond d_text_off[n] is written


def render_and_compare(al, a, cases, only, shifts=(0, 1, 2, 3)):
    """the text of arrays `a` into a poisoned buffer at every shift, against the restatement over `cases` and against the host
    entry; the inputs unchanged.  Returns the device tensors."""
    import torch
    want = D.expected(cases, only)
    ins = inputs(a)
    before = [t.clone() for t in ins]
    n, total = len(a["status"]), len(want[0])
    for shift in shifts:
        text = text_buf(total + 61, shift)
        off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
        out = tensors(al, ins, only_aligned=bool(only), out=(text, off))
        assert out[0] is text and out[1] is off
        assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])
        same_text(text, want[0], total)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))    # the inputs are only read
    h_text, h_off = host(a, only)
    assert np.array_equal(h_text, want[0]) and np.array_equal(h_off, want[1])
    return ins


def pick(cases, n):
    """n of the cases: the multi-round, long-op and seam pairs first, so that the smallest batches hold them; past the set the pairs
    of up to 1 025 columns repeat"""
    ops_n = lambda c: len(c[1] or [])
    cols = lambda c: A.consumed(c[1] or [])[0]
    first = [c for c in cases if ops_n(c) == 200][:1] + [c for c in cases if cols(c) > 5000] + [c for c in cases if ops_n(c) in (65, 129)]
    pool = first + [c for c in cases if not any(c is f for f in first)]
    small = [c for c in pool if cols(c) <= 1025]
    return pool[:n] + [small[i % len(small)] for i in range(max(0, n - len(pool)))]
