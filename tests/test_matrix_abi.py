"""CPU: the score-matrix entry (include/wfa_hip.h: wfahip_score_matrix) is declared, exported and bound, and validates its
arguments before it touches a device; the Python methods and the CLI flag exist."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matrix_entry_declared_exported_and_bound(built):
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    assert "wfahip_score_matrix" in set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    assert "wfahip_score_matrix" in _lib.EXPORTS
    f = _lib.lib().wfahip_score_matrix
    assert f.restype is C.c_int
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert f.argtypes == [vp, C.POINTER(_lib.Params), vp, u64, vp, vp, u64, vp, vp, u64, u32, vp, vp, u64]
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert re.search(r"\bT wfahip_score_matrix$", nm.stdout, flags=re.M)


def _call(ctx=C.c_void_p(1), n_q=2, n_t=3, stride=0, q_off=(0, 4), t_len=(4, 4, 4), status=True, score=True, nulls=()):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    blob = (C.c_uint8 * 8)(*b"ACGTACGT")
    qo = (C.c_uint64 * 2)(*q_off)
    ql = (C.c_uint32 * 2)(4, 4)
    to = (C.c_uint64 * 3)(0, 2, 4)
    tl = (C.c_uint32 * 3)(*t_len)
    st = (C.c_int32 * 64)(*([-7] * 64))
    sc = (C.c_uint32 * 64)(*([7] * 64))
    a = dict(q_off=qo, q_len=ql, t_off=to, t_len=tl)
    for k in nulls:
        a[k] = None
    rc = L.wfahip_score_matrix(ctx, C.byref(prm), blob, 8, a["q_off"], a["q_len"], n_q, a["t_off"], a["t_len"], n_t, 0,
                               st if status else None, sc if score else None, stride)
    assert list(st) == [-7] * 64 and list(sc) == [7] * 64  # nothing written
    return rc


def test_matrix_bad_args_without_device(built):
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG
    assert _call(ctx=None) == BAD
    assert _call(status=False) == BAD
    assert _call(score=False) == BAD
    for k in ("q_off", "q_len", "t_off", "t_len"):
        assert _call(nulls=(k,)) == BAD, k
    assert _call(stride=2) == BAD                    # 0 < out_stride < n_t
    assert _call(q_off=(0, 6)) == BAD                # a query of 4 bases at 6 of an 8-byte blob
    assert _call(t_len=(4, 4, 9)) == BAD             # a target past the end
    assert _call(stride=(1 << 64) - 2) == BAD        # (n_q - 1) * stride + n_t beyond 64 bits
    # an empty or too-long sequence is not checked against the blob (wfahip_score_batch's rule); zero rows or columns: OK, nothing written
    assert _call(n_q=0, nulls=("q_off", "q_len")) == _lib.OK
    assert _call(n_t=0, nulls=("t_off", "t_len")) == _lib.OK


def test_matrix_bad_params_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)  # mismatch 0: check_params refuses it
    blob = (C.c_uint8 * 4)(*b"ACGT")
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(4)
    st, sc = (C.c_int32 * 1)(), (C.c_uint32 * 1)()
    assert L.wfahip_score_matrix(C.c_void_p(1), C.byref(prm), blob, 4, off, ln, 1, off, ln, 1, 0, st, sc, 0) == _lib.ERR_UNSUPPORTED
    assert L.wfahip_score_matrix(C.c_void_p(1), None, blob, 4, off, ln, 1, off, ln, 1, 0, st, sc, 0) == _lib.ERR_BAD_ARG


def test_python_methods_and_cli_flag(built):
    import wfa_amd
    for name in ("score_matrix_arrays", "ScoreMatrix"):
        assert callable(getattr(wfa_amd.Aligner, name))
    r = subprocess.run([sys.executable, "-m", "wfa_amd.cli", "-h"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and re.search(r"^\s*-S\b", r.stdout, flags=re.M), r.stdout


def test_score_matrix_arrays_rejects_bad_input_before_the_call(built):
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: every case below is refused before the C entry is reached)
    blob = np.frombuffer(b"ACGTACGT", np.uint8)
    off, ln = np.array([0, 4], np.uint64), np.array([4, 4], np.uint32)
    with pytest.raises(ValueError):
        al.score_matrix_arrays(blob, off[:1], ln, off, ln)
    with pytest.raises(ValueError):
        al.score_matrix_arrays(blob, off, ln, off, ln, max_score=1 << 32)
    with pytest.raises(ValueError):
        al.score_matrix_arrays(blob, off, ln, off, ln, out=(np.zeros((2, 2), np.int32), np.zeros((2, 3), np.uint32)))
    with pytest.raises(ValueError):
        al.score_matrix_arrays(blob, off, ln, off, ln, out=(np.zeros((2, 2), np.int64), np.zeros((2, 2), np.uint32)))
    with pytest.raises(ValueError):  # row strides differ
        al.score_matrix_arrays(blob, off, ln, off, ln, out=(np.zeros((2, 4), np.int32)[:, :2], np.zeros((2, 2), np.uint32)))
    with pytest.raises(ValueError):  # not contiguous within a row
        al.score_matrix_arrays(blob, off, ln, off, ln, out=(np.zeros((2, 4), np.int32)[:, ::2], np.zeros((2, 4), np.uint32)[:, ::2]))
    with pytest.raises(ValueError):
        al.score_matrix_arrays(blob, off, ln, off, ln, out=np.zeros((2, 2), np.int32))
