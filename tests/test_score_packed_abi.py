"""CPU: the packed score-only entry (include/wfa_hip.h: wfahip_score_batch_packed) is declared, exported, bound, has its Python
method, and rejects bad arguments before it touches a context or a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_declared_and_exported(built):
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    assert "wfahip_score_batch_packed" in declared
    assert "wfahip_score_batch_packed" in _lib.EXPORTS
    assert getattr(_lib.lib(), "wfahip_score_batch_packed") is not None
    # the argument list the issue gives: the packed alignment entry's, with max_score and a wfahip_scores
    m = re.search(r"wfahip_score_batch_packed\s*\(([^)]*)\)", hdr)
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["ctx", "p", "packed", "n_words", "q_woff", "q_len", "t_woff", "t_len", "n_pairs", "max_score", "out"]


def test_header_says_offsets_may_repeat():
    txt = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    doc = txt[:txt.index("int  wfahip_score_batch_packed")]
    doc = doc[doc.rindex("/*"):]
    assert re.search(r"may\s+REPEAT", doc, flags=re.I) and "any order" in doc and "pad" in doc


def test_python_method(built):
    import inspect
    import wfa_amd
    f = wfa_amd.Aligner.score_arrays_packed
    assert callable(f)
    assert list(inspect.signature(f).parameters)[1:] == ["packed", "q_woff", "q_len", "t_woff", "t_len", "max_score"]
    assert inspect.signature(f).parameters["max_score"].default == 0


def test_bad_args_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    words = (C.c_uint32 * 4)(0x1B, 0, 0x1B, 0)  # "ACTG" twice, each with its pad word
    qw = (C.c_uint64 * 1)(0)
    tw = (C.c_uint64 * 1)(2)
    ln = (C.c_uint32 * 1)(4)
    out = _lib.Scores()
    out.n = 99
    f = L.wfahip_score_batch_packed
    assert f(None, C.byref(prm), words, 4, qw, ln, tw, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    assert f(C.c_void_p(1), C.byref(prm), words, 4, qw, ln, tw, ln, 1, 0, None) == _lib.ERR_BAD_ARG
    # (everything below fails before the context -- here the address 1 -- is dereferenced)
    assert f(C.c_void_p(1), None, words, 4, qw, ln, tw, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    out.n = 99
    assert f(C.c_void_p(1), C.byref(prm), None, 4, qw, ln, tw, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    assert out.n == 0 and not out.status and not out.score
    assert f(C.c_void_p(1), C.byref(prm), words, 4, None, ln, tw, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    assert f(C.c_void_p(1), C.byref(prm), words, 4, qw, ln, tw, None, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    # a pair whose words (pad word included) end past n_words, and a hostile 64-bit offset
    assert f(C.c_void_p(1), C.byref(prm), words, 3, qw, ln, tw, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    far = (C.c_uint64 * 1)(1 << 63)
    assert f(C.c_void_p(1), C.byref(prm), words, 4, far, ln, tw, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    far = (C.c_uint64 * 1)((1 << 64) - 1)
    assert f(C.c_void_p(1), C.byref(prm), words, 4, qw, ln, far, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    # then the params, as wfahip_align_batch checks them; and an empty batch is fine without a device
    bad = _lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    assert f(C.c_void_p(1), C.byref(bad), words, 4, qw, ln, tw, ln, 1, 0, C.byref(out)) == _lib.ERR_UNSUPPORTED
    out.n = 99
    assert f(C.c_void_p(1), C.byref(prm), None, 0, None, None, None, None, 0, 0, C.byref(out)) == 0
    assert out.n == 0 and not out.status and not out.score
    L.wfahip_scores_free(C.byref(out))
