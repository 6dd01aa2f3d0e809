"""CPU: the score-only entry (include/wfa_hip.h: wfahip_score_batch / wfahip_scores_free) is declared, exported, bound and
validates its arguments before it touches a device; the Python methods and the CLI flag exist."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_entry_declared_and_exported(built):
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in ("wfahip_score_batch", "wfahip_scores_free"):
        assert name in declared and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None
    assert "WFAHIP_PAIR_OVER_MAX  = 8" in hdr and _lib.PAIR_OVER_MAX == 8


def test_scores_layout(built):
    from wfa_amd import _lib
    assert C.sizeof(_lib.Scores) == 24
    assert [f[0] for f in _lib.Scores._fields_] == ["n", "status", "score"]


def test_score_batch_bad_args_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    blob = (C.c_uint8 * 8)(*b"ACGTACGT")
    off = (C.c_uint64 * 1)(0)
    ln = (C.c_uint32 * 1)(4)
    out = _lib.Scores()
    out.n = 99
    assert L.wfahip_score_batch(None, C.byref(prm), blob, 8, off, ln, off, ln, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    assert L.wfahip_score_batch(C.c_void_p(1), C.byref(prm), blob, 8, off, ln, off, ln, 1, 0, None) == _lib.ERR_BAD_ARG
    L.wfahip_scores_free(None)
    L.wfahip_scores_free(C.byref(out))  # (a zeroed struct is a no-op)
    assert out.n == 0


def test_python_methods_and_cli_flag(built):
    import wfa_amd
    for name in ("score_arrays", "ScoreBatch", "Score"):
        assert callable(getattr(wfa_amd.Aligner, name))
    r = subprocess.run([sys.executable, "-m", "wfa_amd.cli", "-h"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and re.search(r"^\s*-s\b", r.stdout, flags=re.M), r.stdout
