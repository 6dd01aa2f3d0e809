"""CPU: the difference string (include/wfa_hip.h: wfahip_diff_text_device, wfahip_diff_text_packed_device, wfahip_diff_text,
wfahip_diff_text_packed).  The entries' declarations and bindings; the reference README's known answer; the host renderers -- the same
header functions as the kernels -- against the Python restatement of tests/diff_cases.py on the synthetic cases, from bytes and from
words on both strands; every check next to the same input at its bound; the argument checks all four entries make before a context
or a device is touched; the round trip target + string -> query over the oracle's alignments of tests/check_batches.py; and the rule
as a stand-alone program under the host sanitizers (tests/diff_host_test.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import altext_cases as A  # noqa: E402
import altext_pk_cases as P  # noqa: E402
import check_batches as B  # noqa: E402
import cigar_cases as K  # noqa: E402
import diff_cases as D  # noqa: E402


def _results(a, null=()):
    from wfa_amd import _lib
    r = _lib.Results()
    r.n, r.n_ops = len(a["status"]), len(a["ops"])
    r.status = a["status"].ctypes.data_as(C.POINTER(C.c_int32))
    r.ops_off = a["ops_off"].ctypes.data_as(C.POINTER(C.c_uint64))
    r.ops_len = a["ops_len"].ctypes.data_as(C.POINTER(C.c_uint32))
    r.ops = a["ops"].ctypes.data_as(C.POINTER(C.c_uint64))
    r.qbegin, r.qend, r.tbegin, r.tend = (w.ctypes.data_as(C.POINTER(C.c_int32)) for w in a["win"])
    for f in null:
        if hasattr(r, f):
            setattr(r, f, None)
    return r


def _call(a, only, n_threads, null=(), flags=True, size=None):
    """wfahip_diff_text on altext_cases.arrays' dict, or wfahip_diff_text_packed on altext_pk_cases.arrays': (return code, the struct
    -- the caller frees it).  The blob or the words are handed over in a buffer of exactly the size the entry is told of."""
    from wfa_amd import _lib
    r = _results(a, null)
    vp = lambda name, x: None if name in null else x.ctypes.data_as(C.c_void_p)
    cig = _lib.Cigars()
    cig.n = cig.n_bytes = 99
    if "pk" in a:
        words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
        n_words = a.get("n_words", len(words)) if size is None else size
        told = np.ascontiguousarray(words[:n_words]) if n_words <= len(words) else words
        rc = _lib.lib().wfahip_diff_text_packed(C.byref(r), vp("packed", told), n_words, vp("q_woff", q_woff), vp("q_len", q_len),
                                                vp("t_woff", t_woff), vp("t_len", t_len), vp("q_rc", q_rc) if flags else None, only, n_threads,
                                                C.byref(cig))
    else:
        blob, q_off, q_len, t_off, t_len = a["seqs"]
        n_bytes = len(blob) if size is None else size
        told = np.ascontiguousarray(blob[:n_bytes]) if n_bytes <= len(blob) else blob
        rc = _lib.lib().wfahip_diff_text(C.byref(r), vp("blob", told), n_bytes, vp("q_off", q_off), vp("q_len", q_len), vp("t_off", t_off),
                                         vp("t_len", t_len), only, n_threads, C.byref(cig))
    return rc, cig


def _check(cig, cases, only):
    from wfa_amd import _lib
    try:
        text, off = D.expected(cases, only)
        n, nb = len(cases), len(text)
        assert cig.n == n and cig.off[0] == 0 and cig.off[n] == cig.n_bytes == nb
        assert np.array_equal(np.ctypeslib.as_array(cig.off, shape=(n + 1,)), off)
        if nb == 0:
            assert not cig.text
        else:
            bad = np.flatnonzero(np.ctypeslib.as_array(cig.text, shape=(nb,)) != text)
            assert bad.size == 0, f"first differing byte {bad[:1]} of {nb}"
    finally:
        _lib.lib().wfahip_cigars_free(C.byref(cig))
    assert cig.n == 0 and cig.n_bytes == 0 and not cig.text and not cig.off


def test_entries_declared_exported_and_bound(built):
    import wfa_amd
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in ("wfahip_diff_text_device", "wfahip_diff_text_packed_device", "wfahip_diff_text", "wfahip_diff_text_packed"):
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_diff_text_device") == ["ctx", "d_rec", "d_ops", "ops_cap", "d_seq_blob", "blob_bytes", "d_q_off", "d_q_len", "d_t_off",
                                               "d_t_len", "n_pairs", "only_aligned", "d_text", "text_cap", "d_text_off", "text_needed", "stream"]
    assert args("wfahip_diff_text_packed_device") == ["ctx", "d_rec", "d_ops", "ops_cap", "d_packed", "n_words", "d_q_woff", "d_q_len",
                                                      "d_t_woff", "d_t_len", "d_q_rc", "n_pairs", "only_aligned", "d_text", "text_cap",
                                                      "d_text_off", "text_needed", "stream"]
    assert args("wfahip_diff_text") == ["r", "seq_blob", "blob_bytes", "q_off", "q_len", "t_off", "t_len", "only_aligned", "n_threads", "out"]
    assert args("wfahip_diff_text_packed") == ["r", "packed", "n_words", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "only_aligned",
                                               "n_threads", "out"]
    L = _lib.lib()
    assert [len(f.argtypes) for f in (L.wfahip_diff_text_device, L.wfahip_diff_text_packed_device, L.wfahip_diff_text,
                                      L.wfahip_diff_text_packed)] == [17, 18, 10, 11]
    assert L.wfahip_version() == 400
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.diff_tensors) == ["self", "rec", "ops", "blob", "q_off", "q_len", "t_off", "t_len", "only_aligned", "out", "stream"]
    assert sig(wfa_amd.Aligner.diff_tensors_packed) == ["self", "rec", "ops", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc",
                                                        "only_aligned", "out", "stream"]
    assert sig(wfa_amd.diff_text) == ["batch_result", "blob", "q_off", "q_len", "t_off", "t_len", "only_aligned", "n_threads"]
    assert sig(wfa_amd.diff_text_packed) == ["batch_result", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "only_aligned", "n_threads"]
    for f in (wfa_amd.diff_text, wfa_amd.diff_text_packed):
        p = inspect.signature(f).parameters
        assert p["n_threads"].default == 8 and p["only_aligned"].default is False
    for f in (wfa_amd.Aligner.diff_tensors, wfa_amd.Aligner.diff_tensors_packed):
        p = inspect.signature(f).parameters
        assert p["only_aligned"].default is False and p["out"].default is None and p["stream"].default is None
    assert inspect.signature(wfa_amd.diff_text_packed).parameters["q_rc"].default is None


def _batch_result(a):
    import wfa_amd
    z = np.zeros(len(a["status"]), np.uint32)
    qbegin, qend, tbegin, tend = a["win"]
    return wfa_amd.BatchResult(a["status"], z, tbegin, tend, qbegin, qend, z, z, z, z, a["ops_off"], a["ops_len"], a["ops"])


def test_readme_known_answer(built):
    """the reference README's first example: ACCATACTCG against AGGATGCTCG, 1M2X2M1X4M"""
    import wfa_amd
    case = (D.OK, [D.op("M", 1), D.op("X", 2), D.op("M", 2), D.op("X", 1), D.op("M", 4)], b"ACCATACTCG", b"AGGATGCTCG", 1, 10, 1, 10)
    want = b":1*gc*gc:2*ga:4"
    assert D.diff_of(case, 0) == D.diff_of(case, 1) == want and D.apply_diff(case[3], want) == case[2] and D.match_counts(want) == 7
    a = A.arrays([case])
    for only in (False, True):
        text, off = wfa_amd.diff_text(_batch_result(a), *a["seqs"], only_aligned=only)
        assert text.tobytes() == want and off.tolist() == [0, len(want)] and text.dtype == np.uint8 and off.dtype == np.uint64
        for flag in (0, 1):
            pk = P.arrays([case], [flag])
            text, off = wfa_amd.diff_text_packed(_batch_result(pk), *pk["pk"], only_aligned=only, n_threads=1)
            assert text.tobytes() == want and off.tolist() == [0, len(want)]


def test_case_set_is_what_it_claims():
    """the seams the restatement is there for (and, of itself: the inverse on what it renders)"""
    cases = D.cases()
    ops_of = [[(chr(int(o) >> 32), int(o) & 0xFFFFFFFF) for o in (c[1] or [])] for c in cases]
    flat = [x for ops in ops_of for x in ops]
    assert {len(str(n)) for letter, n in flat if letter == "M" and n} >= {1, 2, 3, 4, 5}
    for letter in "IDH":
        assert {n for l2, n in flat if l2 == letter} >= {15, 16, 17, D.LONG}
    assert {n for letter, n in flat if letter == "X"} >= {1, 2, 5, 6, 7, D.LONG} and ("M", D.LONG) in flat
    # an X run of at least four columns starts at every residue of a 4-byte group within its pair's text
    size = lambda letter, n: 0 if n == 0 else 1 + len(str(n)) if letter == "M" else 3 * n if letter == "X" else 1 + n if letter in "IDH" else 0
    starts = set()
    for c, ops in zip(cases, ops_of):
        at = 0
        for letter, n in ops:
            if letter == "X" and n >= 4 and c[0] == D.OK:
                starts.add(at % 4)
            at += size(letter, n)
        assert c[0] != D.OK or at == len(D.diff_of(c, 0))
    assert starts == {0, 1, 2, 3}
    seen = set(b"".join(c[2] + c[3] for c in cases))
    assert len(seen) == 256
    text = D.diff_of(cases[-1], 1)
    assert text == b":1*m@*n[*n`*\x00{-\xff\x7f\x80zzaa~-:1"
    # the inverse, by hand (the synthetic M ops cover random bases: only a real alignment goes round, further down)
    assert D.apply_diff(b"ACGTACGT", b":2*ga+tt:1-ac:2") == b"ACATTTGT" and D.match_counts(b":2*ga+tt:1-ac:2") == 5
    for wrong in (b":2*ca+tt:1-ac:2", b":2*ga+tt:1-ag:2", b":2*ga+tt:1-ac:3", b":2*ga+tt:1-ac:1", b":2*ga+tt:1-ac:2x"):
        with pytest.raises(AssertionError):
            D.apply_diff(b"ACGTACGT", wrong)


@pytest.mark.parametrize("n_threads", [1, 8])
@pytest.mark.parametrize("only_aligned", [0, 1])
def test_host_renderer_on_synthetic_cases_bytes(built, only_aligned, n_threads):
    cases = D.cases()
    a = A.arrays(cases)
    rc, cig = _call(a, only_aligned, n_threads)
    assert rc == 0
    _check(cig, cases, only_aligned)
    b = A.arrays(cases)  # the inputs were only read
    for k in ("status", "ops_off", "ops_len", "ops"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["seqs"] + a["win"], b["seqs"] + b["win"]))


@pytest.mark.parametrize("n_threads", [1, 8])
@pytest.mark.parametrize("only_aligned", [0, 1])
@pytest.mark.parametrize("flags", ["none", "all", "alt"])
def test_host_renderer_on_synthetic_cases_words(built, flags, only_aligned, n_threads):
    cases = P.with_acgt(D.cases())
    fl = P.flags_of(flags, len(cases))
    a = P.arrays(cases, fl)
    rc, cig = _call(a, only_aligned, n_threads)
    assert rc == 0
    _check(cig, cases, only_aligned)
    b = P.arrays(cases, fl)  # the inputs were only read
    for k in ("status", "ops_off", "ops_len", "ops"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["pk"] + a["win"], b["pk"] + b["win"]))
    if flags == "none":  # a null flag array is the array of zeros
        rc, cig = _call(a, only_aligned, n_threads, flags=False)
        assert rc == 0
        _check(cig, cases, only_aligned)


@pytest.mark.parametrize("only_aligned", [0, 1])
def test_tail_bits_and_pad_words_do_not_count(built, only_aligned):
    cases = P.with_acgt(D.cases())
    fl = P.flags_of("alt", len(cases))
    clean = P.arrays(cases, fl)
    for seed in (5, 6):
        junk = P.arrays(cases, fl, junk_tails=seed)
        assert not np.array_equal(junk["pk"][0], clean["pk"][0])
        rc, cig = _call(junk, only_aligned, 3)
        assert rc == 0
        _check(cig, cases, only_aligned)


def test_ten_digit_match_run(built):
    """an M op of 1 000 000 007 columns between an X and an I op: ten digits, and not a base of it is read -- query and target are
    one zero-filled buffer that the host never touches between its first and its last page"""
    import wfa_amd
    ops, n, _ = D.ten_digit_case(b"\0", b"\0")
    a = dict(status=np.zeros(1, np.int32), ops_off=np.zeros(1, np.uint64), ops_len=np.array([3], np.uint32), ops=np.array(ops, np.uint64),
             win=[np.array([v], np.int32) for v in (3, n - 3, 3, n - 3)])
    off0, len1 = np.zeros(1, np.uint64), np.array([n], np.uint32)
    blob = np.zeros(n, np.uint8)
    for only, want in ((False, D.ten_digit_case(b"\0", b"\0")[2]), (True, b":%d" % D.TEN_DIGITS)):
        text, off = wfa_amd.diff_text(_batch_result(a), blob, off0, len1, off0, len1, only_aligned=only, n_threads=2)
        assert text.tobytes() == want and off.tolist() == [0, len(want)]
    words = np.zeros(P.packed_words(n), np.uint32)
    for flag, q in ((0, b"A"), (1, b"T")):
        for only, want in ((False, D.ten_digit_case(b"A", q)[2]), (True, b":%d" % D.TEN_DIGITS)):
            text, off = wfa_amd.diff_text_packed(_batch_result(a), words, off0, len1, off0, len1, q_rc=np.array([flag], np.uint8),
                                                 only_aligned=only, n_threads=2)
            assert text.tobytes() == want and off.tolist() == [0, len(want)]


def test_python_wrappers(built):
    import wfa_amd
    cases = P.with_acgt(D.cases())
    a = P.arrays(cases, P.flags_of("alt", len(cases)))
    br = _batch_result(a)
    for only in (False, True):
        got = wfa_amd.diff_text_packed(br, *a["pk"], only_aligned=only, n_threads=3)
        assert all(np.array_equal(g, w) for g, w in zip(got, D.expected(cases, only)))
        assert got[0].dtype == np.uint8 and got[1].dtype == np.uint64
    with pytest.raises(ValueError):
        wfa_amd.diff_text_packed(br, *a["pk"][:5], q_rc=a["pk"][5][:3])
    with pytest.raises(ValueError):
        wfa_amd.diff_text_packed(br, *a["pk"], n_threads=0)
    with pytest.raises(ValueError):
        wfa_amd.diff_text_packed(br, a["pk"][0].reshape(1, -1), *a["pk"][1:])
    b = A.arrays(D.cases())
    with pytest.raises(ValueError):
        wfa_amd.diff_text(_batch_result(b), b["seqs"][0], b["seqs"][1][:2], *b["seqs"][2:])
    with pytest.raises(ValueError):
        wfa_amd.diff_text(_batch_result(b), *b["seqs"], n_threads=0)
    import torch
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    cpu = lambda shape, dt: torch.zeros(shape, dtype=dt)
    with pytest.raises(ValueError):
        al.diff_tensors_packed(cpu((2, 16), torch.int32), cpu(4, torch.int64), cpu(8, torch.int32), cpu(2, torch.int64), cpu(2, torch.int32),
                               cpu(2, torch.int64), cpu(2, torch.int32))   # on the host
    with pytest.raises(ValueError):
        al.diff_tensors(cpu((2, 16), torch.int32), cpu(4, torch.int64), cpu(8, torch.uint8), cpu(2, torch.int64), cpu(2, torch.int32),
                        cpu(2, torch.int64), cpu(2, torch.int32))


def test_host_renderer_checks_bytes(built):
    """every check next to the same input at the bound: WFAHIP_ERR_BAD_ARG with out zeroed, and a pass.  altext_cases.PAIR: 7 query
    and 9 target bytes; untrimmed +q-tt:4*zx+y-uv, trimmed :4"""
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG

    def bad(only, a, **kw):
        rc, cig = _call(a, only, 2, **kw)
        assert rc == BAD and cig.n == 0 and cig.n_bytes == 0 and not cig.text and not cig.off

    def good(only, a, want, **kw):
        rc, cig = _call(a, only, 2, **kw)
        assert rc == 0 and bytes(cig.text[:cig.n_bytes]) == want
        _lib.lib().wfahip_cigars_free(C.byref(cig))
    whole, trimmed = b"+q-tt:4*zx+y-uv", b":4"
    assert D.diff_of(A.PAIR, 0) == whole and D.diff_of(A.PAIR, 1) == trimmed
    one = A.one
    good(0, one(), whole)
    good(1, one(), trimmed)
    # the blob: the later sequence ends somewhere inside it; a blob that ends one byte short of it is refused
    a = one()
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    end = int(max(q_off[0] + q_len[0], t_off[0] + t_len[0]))
    for only in (0, 1):
        good(only, a, [whole, trimmed][only], size=end)
        bad(only, a, size=end - 1)
        bad(only, a, size=0)
        for name in ("q_off", "t_off"):
            bad(only, one(**{name: 1 << 63}))
            bad(only, one(**{name: (1 << 64) - 1}))
            bad(only, one(**{name: len(blob)}))
    # the ops consume one base more than the sequence holds (whole sequences), or than the window holds (trimmed)
    bad(0, one(q_len=6))
    bad(0, one(t_len=8))
    good(1, one(q_len=6), trimmed)
    bad(1, one(qend=4))
    bad(1, one(tend=5))
    bad(1, one(tbegin=4))
    good(1, one(qbegin=1), trimmed)
    # the trim checks
    bad(1, one(qbegin=0))
    bad(1, one(tbegin=0))
    bad(1, one(qbegin=-3))
    bad(1, one(qend=8))
    bad(1, one(tend=10))
    good(1, one(qbegin=4, qend=7), b":4")
    bad(1, one(qbegin=6, qend=4))
    bad(1, one(qbegin=6, qend=5))
    good(0, one(qbegin=0, qend=-1, tbegin=77, tend=-5), whole)
    # an op range one past n_ops
    n_ops = len(a["ops"])
    bad(0, one(ops_off=n_ops - len(A.PAIR[1]) + 1))
    bad(1, one(ops_len=n_ops + 1, ops_off=0))
    bad(0, one(ops_off=1 << 63))
    # null arguments
    for name in ("status", "ops_off", "ops_len", "ops", "blob", "q_off", "q_len", "t_off", "t_len"):
        bad(0, one(), null=(name,))
    for name in ("qbegin", "qend", "tbegin", "tend"):
        bad(1, one(), null=(name,))
        good(0, one(), whole, null=(name,))
    f = _lib.lib().wfahip_diff_text
    cig = _lib.Cigars()
    assert f(None, None, 0, None, None, None, None, 0, 1, C.byref(cig)) == BAD
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, 0, 1, None) == BAD
    # no pairs: a zeroed out whose off holds one 0
    cig.n = 99
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, 1, 4, C.byref(cig)) == 0
    assert cig.n == 0 and cig.n_bytes == 0 and not cig.text and cig.off and cig.off[0] == 0
    _lib.lib().wfahip_cigars_free(C.byref(cig))
    _lib.lib().wfahip_cigars_free(C.byref(cig))


def test_host_renderer_checks_words(built):
    """altext_pk_cases.PAIR on both strands: GACGTCA against TTACGTGCA; untrimmed +g-tt:4*gc+a-ca, trimmed :4"""
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG

    def bad(only, a, **kw):
        rc, cig = _call(a, only, 2, **kw)
        assert rc == BAD and cig.n == 0 and cig.n_bytes == 0 and not cig.text and not cig.off

    def good(only, a, want, **kw):
        rc, cig = _call(a, only, 2, **kw)
        assert rc == 0 and bytes(cig.text[:cig.n_bytes]) == want
        _lib.lib().wfahip_cigars_free(C.byref(cig))
    whole, trimmed = b"+g-tt:4*gc+a-ca", b":4"
    assert D.diff_of(P.PAIR, 0) == whole and D.diff_of(P.PAIR, 1) == trimmed
    for flag in (0, 1):
        one = lambda **kw: P.one(flag, **kw)
        good(0, one(), whole)
        good(1, one(), trimmed)
        n_words = len(one()["pk"][0])
        for only in (0, 1):
            good(only, one(n_words=n_words), [whole, trimmed][only])
            bad(only, one(n_words=n_words - 1))
            bad(only, one(n_words=0))
        a = one()
        words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
        last = "q_woff" if q_woff[0] > t_woff[0] else "t_woff"
        last_len = int(q_len[0] if last == "q_woff" else t_len[0])
        at_bound = n_words - P.packed_words(last_len)
        assert at_bound == int(a["pk"][1 if last == "q_woff" else 3][0])
        for only in (0, 1):
            bad(only, one(**{last: at_bound + 1}))
            bad(only, one(**{last: n_words}))
            bad(only, one(**{last: 1 << 63}))
            bad(only, one(**{last: (1 << 64) - 1}))
        bad(0, one(**{last[0] + "_len": 16 * (P.packed_words(last_len) - 1) + 1}))   # the pad word counts
        bad(0, one(q_len=6))
        bad(0, one(t_len=8))
        good(1, one(q_len=6), trimmed)
        bad(1, one(qend=4))
        bad(1, one(tend=5))
        bad(1, one(tbegin=4))
        good(1, one(qbegin=1), trimmed)
        bad(1, one(qbegin=0))
        bad(1, one(tbegin=0))
        bad(1, one(qbegin=-3))
        bad(1, one(qend=8))
        bad(1, one(tend=10))
        good(1, one(qbegin=4, qend=7), trimmed)
        bad(1, one(qbegin=6, qend=4))
        bad(1, one(qbegin=6, qend=5))
        good(0, one(qbegin=0, qend=-1, tbegin=77, tend=-5), whole)
        n_ops = len(a["ops"])
        bad(0, one(ops_off=n_ops - len(P.PAIR[1]) + 1))
        bad(1, one(ops_len=n_ops + 1, ops_off=0))
        bad(0, one(ops_off=1 << 63))
    # the offsets of a pair that renders nothing are never looked at: not OK, no op, no byte, and trimmed no M op
    for flag in (0, 1):
        cases = [P.PAIR, P.NOT_OK, P.NO_COLUMN, (P.OK, [], b"", b"", 0, 0, 0, 0), (P.OK, [P.op("X", 2), P.op("I", 1)], b"AC", b"GTA", 1, 2, 1, 3)]
        a = P.arrays(cases, [flag] * 5, seed=2)
        words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
        q_woff[2] = t_woff[2] = len(words)                        # no byte: one word beyond, in both modes
        q_len[2] = t_len[2] = 1000
        rc, cig = _call(a, 0, 2)
        assert rc == 0
        _check(cig, cases, 0)
        q_woff[4] = len(words) - 1                                # no M op: ignored trimmed, refused untrimmed
        rc, cig = _call(a, 1, 2)
        assert rc == 0
        _check(cig, cases, 1)
        bad(0, a)
    for name in ("status", "ops_off", "ops_len", "ops", "packed", "q_woff", "q_len", "t_woff", "t_len"):
        bad(0, P.one(), null=(name,))
    for name in ("qbegin", "qend", "tbegin", "tend"):
        bad(1, P.one(), null=(name,))
        good(0, P.one(), whole, null=(name,))
    good(0, P.one(), whole, null=("q_rc",))
    f = _lib.lib().wfahip_diff_text_packed
    cig = _lib.Cigars()
    assert f(None, None, 0, None, None, None, None, None, 0, 1, C.byref(cig)) == BAD
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, None, 0, 1, None) == BAD
    cig.n = 99
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, None, 1, 4, C.byref(cig)) == 0
    assert cig.n == 0 and cig.n_bytes == 0 and not cig.text and cig.off and cig.off[0] == 0
    _lib.lib().wfahip_cigars_free(C.byref(cig))


def test_ops_of_wf_adaptive_that_overrun_the_sequences_are_refused(built):
    """pair 61 309 of the benchmark's 1 kbp batch: under wf-adaptive the reference's ops consume one base more than both sequences
    hold (tests/test_altext_abi.py restates it).  Untrimmed: BAD_ARG.  Trimmed the windows are the record's and the string renders"""
    import wfa_amd
    from oracle import oracle as O
    from wfa_amd import _lib
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=3, n_pairs=3, length=1000, error_rate=0.05, first_index=61308)
    b = blob.tobytes()
    qs = [b[int(o):int(o) + int(n)] for o, n in zip(q_off, q_len)]
    ts = [b[int(o):int(o) + int(n)] for o, n in zip(t_off, t_len)]
    arrays = wfa_amd.make_blob(qs, ts)
    w = O.align_batch(O.make_params(global_alignment=True, adaptive=(10, 50, 1)), *arrays)
    cases = [(0, [int(x) for x in w.pair_ops(i)], qs[i], ts[i], int(w.qbegin[i]), int(w.qend[i]), int(w.tbegin[i]), int(w.tend[i])) for i in range(3)]
    assert A.consumed(cases[1][1])[1:] == (len(qs[1]) + 1, len(ts[1]) + 1)
    br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions, w.ops_off,
                             w.ops_len, w.ops)
    for call in (lambda **kw: wfa_amd.diff_text(br, *arrays, **kw), lambda **kw: wfa_amd.diff_text_packed(br, *P.pack(cases, [0, 1, 0]), **kw)):
        with pytest.raises(_lib.WfaHipError) as ei:
            call()
        assert ei.value.code == _lib.ERR_BAD_ARG
        got = call(only_aligned=True)
        assert all(np.array_equal(g, x) for g, x in zip(got, D.expected(cases, 1)))


def test_device_entries_bad_args_without_device(built):
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG
    ctx, p = C.c_void_p(1), C.c_void_p(4096)  # (everything below returns before the context -- the address 1 -- or a buffer is dereferenced)
    for f, packed in ((_lib.lib().wfahip_diff_text_device, 0), (_lib.lib().wfahip_diff_text_packed_device, 1)):
        need = C.c_uint64(99)
        ok = [ctx, p, p, 8, p, 8, p, p, p, p] + [p] * packed + [1, 0, p, 8, p, C.byref(need), None]
        N, TEXT, CAP, OFF, NEED = (x + packed for x in (10, 12, 13, 14, 15))

        def call(**kw):
            a = list(ok)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return f(*a)
        at = lambda i: "a%d" % i
        assert call(a0=None) == BAD
        for k in (1, OFF, 6, 7, 8, 9):                       # d_rec, d_text_off, the offset and length arrays
            assert call(**{at(k): None}) == BAD, k
        assert call(a2=None) == BAD                          # d_ops null with ops_cap > 0
        assert call(a4=None) == BAD                          # the blob or the words null with a size > 0
        assert call(**{"a4": None, at(N): 0}) == BAD         # ... whatever n_pairs is
        assert call(**{at(TEXT): None}) == BAD               # a null text with text_cap > 0
        assert call(**{at(TEXT): None, at(N): 0}) == BAD
        assert call(**{at(N): 0xFFFFFFF1}) == BAD
        assert need.value == 99
        # an empty batch without an offset array touches nothing; the flags may be null
        kw = {at(k): None for k in (1, 2, 4, 6, 7, 8, 9, TEXT, OFF)}
        kw.update({"a3": 0, "a5": 0, at(N): 0, at(CAP): 0})
        if packed:
            kw["a10"] = None
        assert call(**kw) == 0 and need.value == 0
        assert call(**{at(N): 0, at(OFF): None, at(NEED): None}) == 0


@pytest.mark.parametrize("name", ["global 300", "global 1k", "semi-global 200"])
def test_round_trip_over_the_oracles_alignments(built, name):
    """for every OK pair whose M columns all match (no M_DIFFERS under check_alignments): trimmed, the target's window and the string
    give the query's window back, and the string's :n counts sum to the record's matches.  From bytes and from words, where every
    second query is stored as its reverse complement."""
    import wfa_amd
    b = B.batch(name)
    w, seqs = b["oracle"], b["seqs"]
    br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions, w.ops_off,
                             w.ops_len, w.ops)
    chk, _, _ = wfa_amd.check_alignments(br, *seqs, penalties=wfa_amd.Penalties(*b["prm"][:3]),
                                         options=wfa_amd.Options(GlobalAlignment=bool(b["prm"][3])))
    text, off = wfa_amd.diff_text(br, *seqs, only_aligned=True)
    text_pk, off_pk = wfa_amd.diff_text_packed(br, *B.packed(b), only_aligned=True, n_threads=3)
    assert np.array_equal(text, text_pk) and np.array_equal(off, off_pk)
    raw, t8 = seqs[0].tobytes(), text.tobytes()
    blob, q_off, q_len, t_off, t_len = seqs
    n_checked = 0
    for i in range(len(w.status)):
        if w.status[i] != 0 or chk[i, 0] & wfa_amd.CHK_M_DIFFERS:
            continue
        s = t8[int(off[i]):int(off[i + 1])]
        q = raw[int(q_off[i]) + int(w.qbegin[i]) - 1:int(q_off[i]) + int(w.qend[i])]
        t = raw[int(t_off[i]) + int(w.tbegin[i]) - 1:int(t_off[i]) + int(w.tend[i])]
        assert D.apply_diff(t, s) == q, i
        assert D.match_counts(s) == int(w.matches[i]), i
        n_checked += 1
    assert n_checked >= len(w.status) - 2 and len(t8) > 20 * n_checked
    # untrimmed and trimmed agree where the ops begin and end with an M op (global alignments mostly do)
    if b["prm"][3]:
        whole = wfa_amd.diff_text(br, *seqs, only_aligned=False, n_threads=1)
        both_m = [i for i in range(len(w.status)) if (int(w.pair_ops(i)[0]) >> 32) == ord("M") == (int(w.pair_ops(i)[-1]) >> 32)]
        w8 = whole[0].tobytes()
        assert len(both_m) > len(w.status) // 2
        assert all(w8[int(whole[1][i]):int(whole[1][i + 1])] == t8[int(off[i]):int(off[i + 1])] for i in both_m)


def test_rule_under_sanitizers():
    src = os.path.join(ROOT, "tests", "diff_host_test.cpp")
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    for name, flags in (("diff_host_test", []), ("diff_host_test_asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(ROOT, "build", name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "diff host test ok" in r.stdout
