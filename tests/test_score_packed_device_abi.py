"""CPU: the screen on device-resident words and its survivors (include/wfa_hip.h: wfahip_score_batch_packed_device,
wfahip_select_pairs_device).  Their declarations, exports and bindings; the argument checks they promise to make before the context is
dereferenced -- with a null context and with a context pointer that cannot be dereferenced --; and the Python mirrors' signatures and
the ValueErrors they raise before the library is called."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_declared_exported_and_bound(built):
    import wfa_amd
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in ("wfahip_score_batch_packed_device", "wfahip_select_pairs_device"):
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_score_batch_packed_device") == ["ctx", "p", "d_packed", "n_words", "d_q_woff", "d_q_len", "d_t_woff", "d_t_len",
                                                        "d_q_rc", "n_pairs", "max_len", "max_score", "d_status", "d_score", "stream"]
    assert args("wfahip_select_pairs_device") == ["ctx", "d_status", "n_pairs", "d_q_off", "d_q_len", "d_t_off", "d_t_len", "d_q_rc", "d_idx",
                                                  "d_q_off_out", "d_q_len_out", "d_t_off_out", "d_t_len_out", "d_q_rc_out", "n_selected",
                                                  "stream"]
    L = _lib.lib()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert L.wfahip_score_batch_packed_device.restype is C.c_int
    assert L.wfahip_score_batch_packed_device.argtypes == [vp, C.POINTER(_lib.Params), vp, u64, vp, vp, vp, vp, vp, u64, u32, u32, vp, vp, vp]
    assert L.wfahip_select_pairs_device.restype is C.c_int
    assert L.wfahip_select_pairs_device.argtypes == [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.score_tensors_packed) == ["self", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "max_score", "out",
                                                         "stream"]
    prm = inspect.signature(wfa_amd.Aligner.score_tensors_packed).parameters
    assert prm["q_rc"].default is None and prm["max_score"].default == 0 and prm["out"].default is None and prm["stream"].default is None
    assert sig(wfa_amd.Aligner.select_tensors) == ["self", "status", "q_off", "q_len", "t_off", "t_len", "q_rc", "stream"]
    prm = inspect.signature(wfa_amd.Aligner.select_tensors).parameters
    assert prm["q_rc"].default is None and prm["stream"].default is None


@pytest.mark.parametrize("ctx", [None, 1])
def test_score_entry_bad_args_before_the_context(built, ctx):
    """ctx = 1: everything below returns before the context -- the address 1 -- or a buffer is dereferenced"""
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_score_batch_packed_device, _lib.ERR_BAD_ARG
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    p = C.c_void_p(4096)
    ok = lambda: [C.c_void_p(ctx), C.byref(prm), p, 64, p, p, p, p, None, 1, 0, 0, p, p, None]
    if ctx is None:
        assert f(*ok()) == BAD
        return
    a = ok()
    a[1] = None  # p
    assert f(*a) == BAD
    for k in (4, 5, 6, 7, 12, 13):  # with n_pairs > 0: a null offset, length or output pointer
        a = ok()
        a[k] = None
        assert f(*a) == BAD, k
    a = ok()
    a[2] = None  # a null d_packed with n_words > 0
    assert f(*a) == BAD
    a = ok()
    a[2], a[9] = None, 0  # ... whatever n_pairs is
    assert f(*a) == BAD
    a = ok()
    a[9] = 0xFFFFFFF1  # n_pairs beyond the limit
    assert f(*a) == BAD
    a = ok()
    a[3] = (1 << 58) + 1  # n_words beyond the limit
    assert f(*a) == BAD
    a[9] = 0  # ... whatever n_pairs is
    assert f(*a) == BAD
    # then the params, as wfahip_align_batch checks them
    bad = _lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    a = ok()
    a[1] = C.byref(bad)
    assert f(*a) == _lib.ERR_UNSUPPORTED
    a[9] = 0  # (before the empty batch is accepted)
    assert f(*a) == _lib.ERR_UNSUPPORTED
    bad = _lib.Params(4, 6, 2, 1, 1, (0, 0), 0, 50, 1)  # wf-adaptive with min_wf_len 0
    a[1] = C.byref(bad)
    assert f(*a) == BAD
    # an empty batch is fine without a device
    assert f(C.c_void_p(ctx), C.byref(prm), None, 0, None, None, None, None, None, 0, 0, 0, None, None, None) == 0
    assert f(C.c_void_p(ctx), C.byref(prm), p, 1 << 58, None, None, None, None, p, 0, 0, 7, None, None, None) == 0


@pytest.mark.parametrize("ctx", [None, 1])
def test_select_entry_bad_args_before_the_context(built, ctx):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_select_pairs_device, _lib.ERR_BAD_ARG
    p = C.c_void_p(4096)
    cnt = C.c_uint64(99)
    ok = lambda: [C.c_void_p(ctx), p, 1, p, p, p, p, p, p, p, p, p, p, p, C.byref(cnt), None]
    if ctx is None:
        assert f(*ok()) == BAD and cnt.value == 99
        return
    a = ok()
    a[14] = None  # n_selected
    assert f(*a) == BAD
    for k in (1, 3, 4, 5, 6, 9, 10, 11, 12):  # with n_pairs > 0: a null status, input or _out array
        a = ok()
        a[k] = None
        assert f(*a) == BAD, k
    for k in (7, 13):  # flags in without flags out, and the reverse
        a = ok()
        a[k] = None
        assert f(*a) == BAD, k
    a = ok()
    a[2] = 0xFFFFFFF1  # n_pairs beyond the limit
    assert f(*a) == BAD
    assert cnt.value == 99
    # an empty batch is fine without a device, with and without flags, and d_idx is optional
    assert f(C.c_void_p(ctx), None, 0, None, None, None, None, None, None, None, None, None, None, None, C.byref(cnt), None) == 0
    assert cnt.value == 0
    cnt.value = 99
    assert f(C.c_void_p(ctx), p, 0, p, p, p, p, p, None, p, p, p, p, p, C.byref(cnt), None) == 0 and cnt.value == 0


def test_python_wrappers_refuse_wrong_inputs_before_the_call(built):
    import torch
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    off, ln = np.array([0, 4], np.uint64), np.array([4, 4], np.uint32)
    cpu = lambda a, dt: torch.from_numpy(a.astype(dt))
    words = np.zeros(12, np.uint32)
    with pytest.raises(ValueError):
        al.score_tensors_packed(words, off, ln, off, ln)                                                                      # numpy arrays
    with pytest.raises(ValueError):
        al.score_tensors_packed(cpu(words, np.int32), cpu(off, np.int64), cpu(ln, np.int32), cpu(off, np.int64), cpu(ln, np.int32))  # on the host
    with pytest.raises(ValueError):
        al.score_tensors_packed(cpu(words, np.int32), cpu(off, np.int64), cpu(ln, np.int32), cpu(off, np.int64), cpu(ln, np.int32),
                                q_rc=np.zeros(2, np.uint8))
    st = np.zeros(2, np.int32)
    with pytest.raises(ValueError):
        al.select_tensors(st, off, ln, off, ln)
    with pytest.raises(ValueError):
        al.select_tensors(cpu(st, np.int32), cpu(off, np.int64), cpu(ln, np.int32), cpu(off, np.int64), cpu(ln, np.int32))
