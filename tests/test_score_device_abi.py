"""CPU: the device-resident score entry (include/wfa_hip.h: wfahip_score_batch_device) and its debug read-back are declared,
exported, bound, and validate their arguments before they touch a device; Aligner.score_tensors exists and refuses host data."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wfahip_score_batch_device", "wfahip_debug_score_device_list")


def test_entry_declared_exported_and_resolvable(built):
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None
    assert _lib.lib().wfahip_version() == 400


def test_bad_args_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    ctx, d = C.c_void_p(1), C.c_void_p(4096)  # (a dummy context and dummy device addresses: none of them may be touched)
    call = lambda c, p, qo, ql, to, tl, st, sc, n=1: L.wfahip_score_batch_device(c, p, d, 8, qo, ql, to, tl, n, 0, 0, st, sc, None)
    assert call(None, C.byref(prm), d, d, d, d, d, d) == _lib.ERR_BAD_ARG
    assert call(ctx, None, d, d, d, d, d, d) == _lib.ERR_BAD_ARG
    for hole in range(6):  # each offset, length and output pointer in turn
        args = [d] * 6
        args[hole] = None
        assert call(ctx, C.byref(prm), *args) == _lib.ERR_BAD_ARG, hole
    assert L.wfahip_score_batch_device(ctx, C.byref(prm), None, 8, d, d, d, d, 1, 0, 0, d, d, None) == _lib.ERR_BAD_ARG
    # the params are checked as the host entry checks them, and an empty batch touches nothing
    assert call(ctx, C.byref(_lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)), d, d, d, d, d, d) == _lib.ERR_UNSUPPORTED
    assert call(ctx, C.byref(prm), None, None, None, None, None, None, n=0) == _lib.OK
    u32p, n = C.POINTER(C.c_uint32)(), C.c_uint64()
    assert L.wfahip_debug_score_device_list(None, C.byref(u32p), C.byref(n), C.byref(u32p), C.byref(n)) == _lib.ERR_BAD_ARG
    assert L.wfahip_debug_score_device_list(ctx, None, C.byref(n), C.byref(u32p), C.byref(n)) == _lib.ERR_BAD_ARG


def test_score_tensors_refuses_host_data(built):
    import torch
    import wfa_amd
    assert callable(wfa_amd.Aligner.score_tensors)
    al = object.__new__(wfa_amd.Aligner)  # (no context: the checks come before the library is called)
    al._device, al._ctx = 0, None
    arrays = wfa_amd.generate_pairs(seed=1, n_pairs=4, length=50, error_rate=0.05)
    with pytest.raises(ValueError):
        al.score_tensors(*arrays)
    tens = [torch.from_numpy(a.view(v)) for a, v in zip(arrays, (np.uint8, np.int64, np.int32, np.int64, np.int32))]
    with pytest.raises(ValueError):
        al.score_tensors(*tens)  # (CPU tensors)
