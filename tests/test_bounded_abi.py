"""CPU: the bounded alignment entries (include/wfa_hip.h: wfahip_align_batch_bounded / wfahip_align_batch_bounded_device) are
declared, exported, bound and validate their arguments before they touch a device; the Python parameters and the CLI flag exist."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wfahip_align_batch_bounded", "wfahip_align_batch_bounded_device")


def test_bounded_entries_declared_and_exported(built):
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS
        fn = getattr(_lib.lib(), name)
        assert fn is not None and fn.restype is C.c_int
    # the unbounded entries' argument lists with one uint32 more
    L = _lib.lib()
    assert len(L.wfahip_align_batch_bounded.argtypes) == len(L.wfahip_align_batch.argtypes) + 1
    assert L.wfahip_align_batch_bounded.argtypes[9] is C.c_uint32
    assert len(L.wfahip_align_batch_bounded_device.argtypes) == len(L.wfahip_align_batch_device.argtypes) + 1
    assert L.wfahip_align_batch_bounded_device.argtypes[10] is C.c_uint32
    assert _lib.PAIR_OVER_MAX == 8 and C.sizeof(_lib.Timing) == 72


def test_bounded_bad_args_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    blob = (C.c_uint8 * 8)(*b"ACGTACGT")
    off = (C.c_uint64 * 1)(0)
    ln = (C.c_uint32 * 1)(4)
    out = _lib.Results()
    fake = C.c_void_p(1)  # (never dereferenced: the null argument is found first)
    assert L.wfahip_align_batch_bounded(None, C.byref(prm), blob, 8, off, ln, off, ln, 1, 100, C.byref(out)) == _lib.ERR_BAD_ARG
    assert L.wfahip_align_batch_bounded(fake, C.byref(prm), blob, 8, off, ln, off, ln, 1, 100, None) == _lib.ERR_BAD_ARG
    needed = C.c_uint64(7)
    assert L.wfahip_align_batch_bounded_device(None, C.byref(prm), blob, 8, off, ln, off, ln, 1, 4, 100, blob, blob, 1,
                                               C.byref(needed), None) == _lib.ERR_BAD_ARG
    assert L.wfahip_align_batch_bounded(fake, None, blob, 8, off, ln, off, ln, 1, 100, C.byref(out)) == _lib.ERR_BAD_ARG
    assert L.wfahip_align_batch_bounded_device(fake, None, blob, 8, off, ln, off, ln, 1, 4, 100, blob, blob, 1,
                                               C.byref(needed), None) == _lib.ERR_BAD_ARG


def test_python_parameters_and_cli_flag(built):
    import wfa_amd
    for name in ("align_arrays", "AlignBatch"):
        prm = inspect.signature(getattr(wfa_amd.Aligner, name)).parameters
        assert "max_score" in prm and prm["max_score"].default == 0
    assert isinstance(wfa_amd.ErrOverMaxScore, wfa_amd.WfaError)
    r = subprocess.run([sys.executable, "-m", "wfa_amd.cli", "-h"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and re.search(r"^\s*-b\b", r.stdout, flags=re.M), r.stdout
    # the C++ and Go mirrors name the entry
    assert "wfahip_align_batch_bounded" in open(os.path.join(ROOT, "wfa_amd", "host", "wfa.hpp")).read()
    assert "AlignBatchBounded" in open(os.path.join(ROOT, "go", "wfa", "wfa.go")).read()
