"""CPU: the reverse-strand score entries (include/wfa_hip.h: wfahip_score_batch_packed_rc, wfahip_score_matrix_rc,
wfahip_revcomp_packed).  wfahip_revcomp_packed against a naive restatement -- bytes, reverse complement, pack -- at every word
boundary and with anything in the bits it must not read as sequence; the two entries' argument checks, made before a context or a
device is touched; and rc_word's read range as a stand-alone program under the host sanitizers (tests/rc_host_test.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(1, 131)) + [2047, 2048, 2049]
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(s):
    return s.translate(COMP)[::-1]


def _pack_seq(s):
    """one sequence as wfahip_pack_pairs writes it: 16 bases per word, code (ascii >> 1) & 3, then the pad word"""
    a = np.frombuffer(s, dtype=np.uint8)
    nw = (len(a) + 15) // 16
    codes = np.zeros(nw * 16, dtype=np.uint64)
    codes[:len(a)] = (a >> 1) & 3
    words = (codes.reshape(nw, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    return np.concatenate([words, np.zeros(1, np.uint32)])


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def test_entries_declared_exported_and_bound(built):
    import inspect
    import wfa_amd
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in ("wfahip_score_batch_packed_rc", "wfahip_score_matrix_rc", "wfahip_revcomp_packed"):
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_score_batch_packed_rc") == ["ctx", "p", "packed", "n_words", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "n_pairs",
                                                    "max_score", "out"]
    assert args("wfahip_score_matrix_rc") == ["ctx", "p", "seq_blob", "blob_bytes", "q_off", "q_len", "n_q", "q_rc", "t_off", "t_len", "n_t",
                                              "max_score", "status", "score", "out_stride"]
    assert args("wfahip_revcomp_packed") == ["src", "len", "dst"]
    assert _lib.lib().wfahip_version() == 400
    # the Python mirror
    assert "q_rc" in inspect.signature(wfa_amd.Aligner.score_arrays_packed_rc).parameters
    assert inspect.signature(wfa_amd.Aligner.score_matrix_arrays).parameters["q_rc"].default is None
    assert inspect.signature(wfa_amd.Aligner.ScoreMatrix).parameters["strands"].default == "+"
    assert callable(wfa_amd.revcomp_packed)


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFF])
def test_revcomp_packed_against_naive(built, fill):
    """the source's tail bits, its pad word and the word behind it all zero / all ones: the same output, tail and pad zero"""
    from wfa_amd import _lib
    rng = np.random.default_rng(31)
    f = _lib.lib().wfahip_revcomp_packed
    for n in LENGTHS:
        s = _rand(rng, n)
        nw, tail = (n + 15) // 16, n % 16
        src = np.concatenate([_pack_seq(s), np.zeros(1, np.uint32)])  # words, pad word, the following word
        if fill:
            if tail:
                src[nw - 1] |= np.uint32((0xFFFFFFFF << (2 * tail)) & 0xFFFFFFFF)
            src[nw:] = fill
        dst = np.full(nw + 3, 0xDEADBEEF, np.uint32)
        assert f(src.ctypes.data_as(C.c_void_p), n, dst[1:].ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(dst[1:nw + 2], _pack_seq(_revcomp(s))), n
        assert dst[0] == 0xDEADBEEF and dst[nw + 2] == 0xDEADBEEF, n  # exactly wfahip_packed_words(n) words written


def test_revcomp_packed_involution_and_palindromes(built):
    import wfa_amd
    rng = np.random.default_rng(32)
    for n in LENGTHS:
        w = _pack_seq(_rand(rng, n))
        assert np.array_equal(wfa_amd.revcomp_packed(wfa_amd.revcomp_packed(w, n), n), w), n
    for k in (1, 3, 4, 5, 16, 33, 512):
        w = _pack_seq(b"ACGT" * k)  # its own reverse complement
        assert np.array_equal(wfa_amd.revcomp_packed(w, 4 * k), w), k
    assert not np.array_equal(wfa_amd.revcomp_packed(_pack_seq(b"AACG"), 4), _pack_seq(b"AACG"))


def test_revcomp_packed_bad_args(built):
    from wfa_amd import _lib
    f = _lib.lib().wfahip_revcomp_packed
    w = (C.c_uint32 * 2)(0x1B, 0)
    d = (C.c_uint32 * 2)(7, 7)
    assert f(w, 4, None) == _lib.ERR_BAD_ARG
    assert f(None, 4, d) == _lib.ERR_BAD_ARG
    assert f(w, (1 << 29), d) == _lib.ERR_BAD_ARG and list(d) == [7, 7]


def test_packed_rc_bad_args_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    words = (C.c_uint32 * 4)(0x1B, 0, 0x1B, 0)
    qw, tw, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(2), (C.c_uint32 * 1)(4)
    flag = (C.c_uint8 * 1)(1)
    out = _lib.Scores()
    out.n = 99
    f = L.wfahip_score_batch_packed_rc
    ctx = C.c_void_p(1)  # (everything below fails before the context -- the address 1 -- is dereferenced)
    assert f(None, C.byref(prm), words, 4, qw, ln, tw, ln, flag, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    assert f(ctx, C.byref(prm), words, 4, qw, ln, tw, ln, flag, 1, 0, None) == _lib.ERR_BAD_ARG
    assert f(ctx, None, words, 4, qw, ln, tw, ln, flag, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    out.n = 99
    assert f(ctx, C.byref(prm), None, 4, qw, ln, tw, ln, flag, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    assert out.n == 0 and not out.status and not out.score
    for null in range(4):
        a = [qw, ln, tw, ln]
        a[null] = None
        assert f(ctx, C.byref(prm), words, 4, *a, flag, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    # a word range outside the buffer, with the flag set, clear and absent: the pad word past the end, hostile offsets
    far = (C.c_uint64 * 1)(1 << 63)
    for fl in (flag, (C.c_uint8 * 1)(0), None):
        assert f(ctx, C.byref(prm), words, 3, qw, ln, tw, ln, fl, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
        assert f(ctx, C.byref(prm), words, 4, far, ln, tw, ln, fl, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
        assert f(ctx, C.byref(prm), words, 4, qw, ln, (C.c_uint64 * 1)((1 << 64) - 1), ln, fl, 1, 0, C.byref(out)) == _lib.ERR_BAD_ARG
    bad = _lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    assert f(ctx, C.byref(bad), words, 4, qw, ln, tw, ln, flag, 1, 0, C.byref(out)) == _lib.ERR_UNSUPPORTED
    # an empty batch is fine without a device, with flags or without
    for fl in (flag, None):
        out.n = 99
        assert f(ctx, C.byref(prm), None, 0, None, None, None, None, fl, 0, 0, C.byref(out)) == 0
        assert out.n == 0 and not out.status and not out.score


def _matrix(ctx=C.c_void_p(1), n_q=2, n_t=3, stride=0, q_off=(0, 4), t_len=(4, 4, 4), status=True, score=True, nulls=(), flags=(1, 0)):
    from wfa_amd import _lib
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    blob = (C.c_uint8 * 8)(*b"ACGTACGT")
    a = dict(q_off=(C.c_uint64 * 2)(*q_off), q_len=(C.c_uint32 * 2)(4, 4), t_off=(C.c_uint64 * 3)(0, 2, 4), t_len=(C.c_uint32 * 3)(*t_len))
    for k in nulls:
        a[k] = None
    st = (C.c_int32 * 64)(*([-7] * 64))
    sc = (C.c_uint32 * 64)(*([7] * 64))
    fl = None if flags is None else (C.c_uint8 * 2)(*flags)
    rc = _lib.lib().wfahip_score_matrix_rc(ctx, C.byref(prm), blob, 8, a["q_off"], a["q_len"], n_q, fl, a["t_off"], a["t_len"], n_t, 0,
                                           st if status else None, sc if score else None, stride)
    assert list(st) == [-7] * 64 and list(sc) == [7] * 64  # nothing written
    return rc


def test_matrix_rc_bad_args_without_device(built):
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG
    for flags in ((1, 0), None):
        assert _matrix(ctx=None, flags=flags) == BAD
        assert _matrix(status=False, flags=flags) == BAD
        assert _matrix(score=False, flags=flags) == BAD
        for k in ("q_off", "q_len", "t_off", "t_len"):
            assert _matrix(nulls=(k,), flags=flags) == BAD, k
        assert _matrix(stride=2, flags=flags) == BAD              # 0 < out_stride < n_t
        assert _matrix(q_off=(0, 6), flags=flags) == BAD          # a query of 4 bases at 6 of an 8-byte blob
        assert _matrix(t_len=(4, 4, 9), flags=flags) == BAD       # a target past the end
        assert _matrix(stride=(1 << 64) - 2, flags=flags) == BAD  # (n_q - 1) * stride + n_t beyond 64 bits
        assert _matrix(n_q=0, nulls=("q_off", "q_len"), flags=flags) == _lib.OK
        assert _matrix(n_t=0, nulls=("t_off", "t_len"), flags=flags) == _lib.OK


def test_python_rejects_bad_flags_before_the_call(built):
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    blob = np.frombuffer(b"ACGTACGT", np.uint8)
    off, ln = np.array([0, 4], np.uint64), np.array([4, 4], np.uint32)
    with pytest.raises(ValueError):
        al.score_matrix_arrays(blob, off, ln, off, ln, q_rc=[1])
    with pytest.raises(ValueError):
        al.score_arrays_packed_rc(np.zeros(4, np.uint32), off, ln, off, ln, [1, 0, 1])
    with pytest.raises(ValueError):
        al.ScoreMatrix([b"ACGT"], strands="-")


def test_best_strand_rule(built):
    import wfa_amd
    OK, OVER, EMPTY = 0, 8, 1
    st_f = np.array([OK, OK, OVER, OK, OVER, EMPTY, OVER], np.int32)
    sc_f = np.array([10, 10, 0, 7, 0, 0, 0], np.uint32)
    st_r = np.array([OK, OK, OK, OVER, OVER, OVER, EMPTY], np.int32)
    sc_r = np.array([4, 10, 30, 0, 0, 0, 0], np.uint32)
    st, sc, strand = wfa_amd.best_strand(st_f, sc_f, st_r, sc_r)
    assert list(st) == [OK, OK, OK, OK, OVER, EMPTY, OVER]
    assert list(sc) == [4, 10, 30, 7, 0, 0, 0]
    assert list(strand) == [1, 0, 1, 0, 0, 0, 0]


def test_rc_word_read_range_under_sanitizers():
    exe = os.path.join(ROOT, "build", "rc_host_test_asan_ubsan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "rc_host_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rc host test ok" in r.stdout
