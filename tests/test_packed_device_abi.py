"""CPU: the packed entries on device-resident input (include/wfa_hip.h: wfahip_pack_pairs_device, wfahip_align_batch_packed_device).
Their declarations, exports and bindings; the argument checks they promise to make before the context is dereferenced -- with a null
context and with a context pointer that cannot be dereferenced --; and the Python mirrors' signatures and the ValueErrors they raise
before the library is called."""
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
    for name in ("wfahip_pack_pairs_device", "wfahip_align_batch_packed_device"):
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_pack_pairs_device") == ["ctx", "d_seq_blob", "blob_bytes", "d_q_off", "d_q_len", "d_t_off", "d_t_len", "n_pairs",
                                                "d_packed", "words_cap", "d_q_woff", "d_t_woff", "n_words", "stream"]
    assert args("wfahip_align_batch_packed_device") == ["ctx", "p", "d_packed", "n_words", "d_q_woff", "d_q_len", "d_t_woff", "d_t_len",
                                                        "d_q_rc", "n_pairs", "max_len", "max_score", "d_rec", "d_ops", "ops_cap",
                                                        "ops_needed", "stream"]
    L = _lib.lib()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert L.wfahip_pack_pairs_device.restype is C.c_int
    assert L.wfahip_pack_pairs_device.argtypes == [vp, vp, u64, vp, vp, vp, vp, u64, vp, u64, vp, vp, C.POINTER(u64), vp]
    assert L.wfahip_align_batch_packed_device.restype is C.c_int
    assert L.wfahip_align_batch_packed_device.argtypes == [vp, C.POINTER(_lib.Params), vp, u64, vp, vp, vp, vp, vp, u64, u32, u32, vp, vp,
                                                           u64, C.POINTER(u64), vp]
    assert L.wfahip_version() == 400
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.pack_tensors) == ["self", "blob", "q_off", "q_len", "t_off", "t_len", "stream"]
    assert sig(wfa_amd.Aligner.align_tensors_packed) == ["self", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "max_score", "stream"]
    prm = inspect.signature(wfa_amd.Aligner.align_tensors_packed).parameters
    assert prm["q_rc"].default is None and prm["max_score"].default == 0 and prm["stream"].default is None
    assert inspect.signature(wfa_amd.Aligner.pack_tensors).parameters["stream"].default is None
    # the kernels' unit is part of the library's build
    assert re.search(r"^UNITS\s*:=.*\bwfa_packdev\b", open(os.path.join(ROOT, "Makefile")).read(), flags=re.M)


@pytest.mark.parametrize("ctx", [None, 1])
def test_pack_entry_bad_args_before_the_context(built, ctx):
    """ctx = 1: everything below returns before the context -- the address 1 -- or a buffer is dereferenced"""
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_pack_pairs_device, _lib.ERR_BAD_ARG
    p = C.c_void_p(4096)
    nw = C.c_uint64(99)
    ok = lambda: [C.c_void_p(ctx), p, 64, p, p, p, p, 1, p, 8, p, p, C.byref(nw), None]
    if ctx is None:
        assert f(*ok()) == BAD and nw.value == 99
        assert f(None, None, 0, None, None, None, None, 0, None, 0, None, None, C.byref(nw), None) == BAD  # ... whatever n_pairs is
        return
    for k in (3, 4, 5, 6, 10, 11):  # with n_pairs > 0: a null offset, length or woff array
        a = ok()
        a[k] = None
        assert f(*a) == BAD, k
    a = ok()
    a[1] = None  # a null blob with blob_bytes > 0
    assert f(*a) == BAD
    a = ok()
    a[8] = None  # a null d_packed with words_cap > 0
    assert f(*a) == BAD
    a = ok()
    a[7] = 0xFFFFFFF1  # n_pairs beyond the limit
    assert f(*a) == BAD
    a = ok()
    a[1], a[7] = None, 0  # ... the two whatever n_pairs is
    assert f(*a) == BAD
    assert nw.value == 99
    # an empty batch touches nothing
    assert f(C.c_void_p(ctx), None, 0, None, None, None, None, 0, None, 0, None, None, C.byref(nw), None) == 0 and nw.value == 0
    assert f(C.c_void_p(ctx), p, 64, None, None, None, None, 0, p, 8, None, None, None, None) == 0


@pytest.mark.parametrize("ctx", [None, 1])
def test_align_entry_bad_args_before_the_context(built, ctx):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_align_batch_packed_device, _lib.ERR_BAD_ARG
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    p = C.c_void_p(4096)
    need = C.c_uint64(99)
    ok = lambda: [C.c_void_p(ctx), C.byref(prm), p, 64, p, p, p, p, None, 1, 0, 0, p, p, 8, C.byref(need), None]
    if ctx is None:
        assert f(*ok()) == BAD and need.value == 99
        return
    a = ok()
    a[1] = None  # p
    assert f(*a) == BAD
    for k in (4, 5, 6, 7, 12):  # with n_pairs > 0: a null offset, length or d_rec pointer
        a = ok()
        a[k] = None
        assert f(*a) == BAD, k
    a = ok()
    a[2] = None  # a null d_packed with n_words > 0
    assert f(*a) == BAD
    a = ok()
    a[13] = None  # a null d_ops with ops_cap > 0
    assert f(*a) == BAD
    a = ok()
    a[2], a[9] = None, 0  # ... the two whatever n_pairs is
    assert f(*a) == BAD
    assert need.value == 99
    # then the params, as wfahip_align_batch checks them
    bad = _lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    a = ok()
    a[1] = C.byref(bad)
    assert f(*a) == _lib.ERR_UNSUPPORTED
    bad = _lib.Params(4, 6, 2, 1, 1, (0, 0), 0, 50, 1)  # wf-adaptive with min_wf_len 0
    a[1] = C.byref(bad)
    assert f(*a) == BAD
    # an empty batch is fine without a device
    assert f(C.c_void_p(ctx), C.byref(prm), None, 0, None, None, None, None, None, 0, 0, 0, None, None, 0, C.byref(need), None) == 0
    assert need.value == 0


def test_python_wrappers_refuse_wrong_inputs_before_the_call(built):
    import torch
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    blob = np.frombuffer(b"ACGTACGT", np.uint8)
    off, ln = np.array([0, 4], np.uint64), np.array([4, 4], np.uint32)
    cpu = lambda a, dt: torch.from_numpy(a.astype(dt))
    with pytest.raises(ValueError):
        al.pack_tensors(blob, off, ln, off, ln)                                                                              # numpy arrays
    with pytest.raises(ValueError):
        al.pack_tensors(cpu(blob, np.uint8), cpu(off, np.int64), cpu(ln, np.int32), cpu(off, np.int64), cpu(ln, np.int32))  # on the host
    words = np.zeros(12, np.uint32)
    with pytest.raises(ValueError):
        al.align_tensors_packed(words, off, ln, off, ln)                                                                    # numpy arrays
    with pytest.raises(ValueError):
        al.align_tensors_packed(cpu(words, np.int32), cpu(off, np.int64), cpu(ln, np.int32), cpu(off, np.int64), cpu(ln, np.int32))
    with pytest.raises(ValueError):
        al.align_tensors_packed(cpu(words, np.int32), cpu(off, np.int64), cpu(ln, np.int32), cpu(off, np.int64), cpu(ln, np.int32),
                                q_rc=np.zeros(2, np.uint8))


@pytest.mark.gpu
def test_python_wrappers_refuse_wrong_dtypes_and_lengths():
    """on the device, where the tensors pass the first check: a wrong dtype for each tensor, arrays of differing lengths, flags that
    are not uint8 or not one per pair, a stream that is none"""
    import torch
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(4, 6, 2), wfa_amd.Options(GlobalAlignment=True), device=0)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).to(dev)
    blob, off, ln = t(np.frombuffer(b"ACGTACGT", np.uint8), np.uint8), t([0, 4], np.int64), t([4, 4], np.int32)
    good = [blob, off, ln, off, ln]
    for k, wrong in ((0, np.int8), (1, np.int32), (2, np.int64), (3, np.int32), (4, np.int64)):
        a = list(good)
        a[k] = t(a[k].cpu().numpy(), wrong)
        with pytest.raises(ValueError):
            al.pack_tensors(*a)
    with pytest.raises(ValueError):
        al.pack_tensors(blob, off[:1], ln, off, ln)
    with pytest.raises(ValueError):
        al.pack_tensors(*good, stream=0)
    packed, qw, tw = al.pack_tensors(*good)
    assert packed.dtype == torch.int32 and qw.dtype == torch.int64 and tw.dtype == torch.int64 and packed.numel() == 4 * 2 + 4
    good = [packed, qw, ln, tw, ln]
    for k, wrong in ((0, np.int64), (1, np.int32), (2, np.int64), (3, np.int32), (4, np.int64)):
        a = list(good)
        a[k] = t(a[k].cpu().numpy(), wrong)
        with pytest.raises(ValueError):
            al.align_tensors_packed(*a)
    with pytest.raises(ValueError):
        al.align_tensors_packed(packed, qw, ln, tw[:1], ln)
    with pytest.raises(ValueError):
        al.align_tensors_packed(*good, q_rc=t([1, 0], np.int32))
    with pytest.raises(ValueError):
        al.align_tensors_packed(*good, q_rc=t([1], np.uint8))
    with pytest.raises(ValueError):
        al.align_tensors_packed(*good, max_score=1 << 32)
    with pytest.raises(ValueError):
        al.align_tensors_packed(*good, stream=0)
    rec, ops = al.align_tensors_packed(*good, q_rc=t([0, 0], np.uint8))
    assert rec.shape == (2, 16) and rec.dtype == torch.int32 and ops.dtype == torch.int64
    al.close()
