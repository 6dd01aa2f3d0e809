"""CPU: the reverse-strand full-alignment entry (include/wfa_hip.h: wfahip_align_batch_packed_rc) is declared, exported, bound and has its
Python method; every whole-call error comes back before the context is dereferenced, with the flags set, clear and NULL; an empty
batch leaves a zeroed result; and the mirror addressing of wfa_rc.hpp holds as a stand-alone program under the host sanitizers
(tests/rc_mirror_host_test.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wfahip_align_batch_packed_rc"


def test_entry_declared_exported_and_bound(built):
    import wfa_amd
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    assert NAME in declared and NAME in _lib.EXPORTS and getattr(_lib.lib(), NAME) is not None
    args = [a.strip().split()[-1].lstrip("*") for a in re.search(NAME + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args == ["ctx", "p", "packed", "n_words", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "n_pairs", "out"]
    assert _lib.lib().wfahip_version() == 400
    f = wfa_amd.Aligner.align_arrays_packed_rc
    assert list(inspect.signature(f).parameters)[1:] == ["packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc"]
    assert list(inspect.signature(wfa_amd.Aligner.align_arrays_packed).parameters)[1:] == ["packed", "q_woff", "q_len", "t_woff", "t_len"]


def _zeroed(out):
    return out.n == 0 and out.n_ops == 0 and not out.status and not out.score and not out.ops and not out.ops_off and not out.ops_len


def test_bad_args_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    words = (C.c_uint32 * 4)(0x1B, 0, 0x1B, 0)  # "ACTG" twice, each with its pad word
    qw, tw, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(2), (C.c_uint32 * 1)(4)
    out = _lib.Results()
    f = getattr(L, NAME)
    ctx = C.c_void_p(1)  # (everything below fails before the context -- the address 1 -- is dereferenced)
    for fl in ((C.c_uint8 * 1)(1), (C.c_uint8 * 1)(0), None):
        assert f(None, C.byref(prm), words, 4, qw, ln, tw, ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        assert f(ctx, C.byref(prm), words, 4, qw, ln, tw, ln, fl, 1, None) == _lib.ERR_BAD_ARG
        out.n = 99
        assert f(ctx, None, words, 4, qw, ln, tw, ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        assert _zeroed(out)
        assert f(ctx, C.byref(prm), None, 4, qw, ln, tw, ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        for null in range(4):
            a = [qw, ln, tw, ln]
            a[null] = None
            assert f(ctx, C.byref(prm), words, 4, *a, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        # a sequence that leaves the buffer, and hostile 64-bit offsets that would wrap a sum around
        assert f(ctx, C.byref(prm), words, 4, (C.c_uint64 * 1)(4), ln, tw, ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        assert f(ctx, C.byref(prm), words, 4, qw, ln, (C.c_uint64 * 1)(5), ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        assert f(ctx, C.byref(prm), words, 4, qw, (C.c_uint32 * 1)(65), tw, ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        assert f(ctx, C.byref(prm), words, 4, (C.c_uint64 * 1)(1 << 63), ln, tw, ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        assert f(ctx, C.byref(prm), words, 4, qw, ln, (C.c_uint64 * 1)((1 << 64) - 1), ln, fl, 1, C.byref(out)) == _lib.ERR_BAD_ARG
        # the params, as wfahip_align_batch checks them
        bad = _lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)
        assert f(ctx, C.byref(bad), words, 4, qw, ln, tw, ln, fl, 1, C.byref(out)) == _lib.ERR_UNSUPPORTED
        assert _zeroed(out)


def test_the_entry_without_flags_has_the_same_errors(built):
    """wfahip_align_batch_packed is the new entry with q_rc = NULL: one copy of the checks"""
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    words = (C.c_uint32 * 4)(0x1B, 0, 0x1B, 0)
    qw, tw, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(2), (C.c_uint32 * 1)(4)
    out = _lib.Results()
    f, ctx = L.wfahip_align_batch_packed, C.c_void_p(1)
    assert f(ctx, C.byref(prm), None, 4, qw, ln, tw, ln, 1, C.byref(out)) == _lib.ERR_BAD_ARG
    assert f(ctx, C.byref(prm), words, 4, (C.c_uint64 * 1)(1 << 63), ln, tw, ln, 1, C.byref(out)) == _lib.ERR_BAD_ARG
    assert f(ctx, C.byref(prm), words, 4, qw, ln, (C.c_uint64 * 1)(5), ln, 1, C.byref(out)) == _lib.ERR_BAD_ARG
    out.n = 99
    assert f(ctx, C.byref(prm), None, 0, None, None, None, None, 0, C.byref(out)) == _lib.OK and _zeroed(out)


def test_empty_batch_gives_a_zeroed_out(built):
    from wfa_amd import _lib
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    f = getattr(_lib.lib(), NAME)
    for fl in ((C.c_uint8 * 1)(1), None):
        out = _lib.Results()
        out.n, out.n_ops = 99, 7
        assert f(C.c_void_p(1), C.byref(prm), None, 0, None, None, None, None, fl, 0, C.byref(out)) == _lib.OK
        assert _zeroed(out)
        _lib.lib().wfahip_results_free(C.byref(out))


def test_python_rejects_bad_flags_before_the_call(built):
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    off, ln = np.array([0, 2], np.uint64), np.array([4, 4], np.uint32)
    with pytest.raises(ValueError):
        al.align_arrays_packed_rc(np.zeros(4, np.uint32), off, ln, off, ln, [1, 0, 1])
    with pytest.raises(ValueError):
        al.align_arrays_packed_rc(np.zeros(4, np.uint32), off[:1], ln, off, ln, [1, 0])


def test_mirror_addresses_under_sanitizers():
    exe = os.path.join(ROOT, "build", "rc_mirror_host_test_asan_ubsan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "rc_mirror_host_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rc mirror host test ok" in r.stdout
