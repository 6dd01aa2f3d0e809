"""CPU: the display rows from 2-bit packed words, both strands (include/wfa_hip.h: wfahip_alignment_text_packed_device,
wfahip_alignment_text_packed).  The entries' declarations and bindings; the host renderer -- the same header functions as the
kernels -- against AlignmentResult.AlignmentText on the synthetic cases of tests/altext_cases.py with ACGT sequences, a flagged query
packed as its reverse complement; every check next to the same input at the bound; the argument checks both entries make before a
context or a device is touched; and the decoding rule as a stand-alone program under the host sanitizers
(tests/altext_pk_host_test.cpp)."""
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


def _call(a, only, n_threads, n_words=None, null=(), flags=True):
    """wfahip_alignment_text_packed on altext_pk_cases.arrays' dict: (return code, the struct -- the caller frees it)"""
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
    words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
    if n_words is None:
        n_words = a.get("n_words", len(words))
    # exactly the words the entry is told of, in a buffer of their own: nothing behind them belongs to the call
    told = np.ascontiguousarray(words[:n_words]) if n_words <= len(words) else words
    vp = lambda name, x: None if name in null else x.ctypes.data_as(C.c_void_p)
    txt = _lib.AlignTexts()
    txt.n = txt.n_bytes = 99
    rc = _lib.lib().wfahip_alignment_text_packed(C.byref(r), vp("packed", told), n_words, vp("q_woff", q_woff), vp("q_len", q_len),
                                                 vp("t_woff", t_woff), vp("t_len", t_len), vp("q_rc", q_rc) if flags else None, only,
                                                 n_threads, C.byref(txt))
    return rc, txt


def _check(txt, cases, only):
    from wfa_amd import _lib
    try:
        want = A.expected(cases, only)
        n, nb = len(cases), len(want[0])
        assert txt.n == n and txt.off[0] == 0 and txt.off[n] == txt.n_bytes == nb
        assert np.array_equal(np.ctypeslib.as_array(txt.off, shape=(n + 1,)), want[3])
        for name, p, w in zip(("q_row", "a_row", "t_row"), (txt.q_row, txt.a_row, txt.t_row), want):
            if nb == 0:
                assert not p
                continue
            bad = np.flatnonzero(np.ctypeslib.as_array(p, shape=(nb,)) != w)
            assert bad.size == 0, f"{name}: first differing byte {bad[:1]} of {nb}"
    finally:
        _lib.lib().wfahip_align_texts_free(C.byref(txt))
    assert txt.n == 0 and txt.n_bytes == 0 and not txt.q_row and not txt.a_row and not txt.t_row and not txt.off


def test_entries_declared_exported_and_bound(built):
    import wfa_amd
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in ("wfahip_alignment_text_packed_device", "wfahip_alignment_text_packed"):
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_alignment_text_packed_device") == ["ctx", "d_rec", "d_ops", "ops_cap", "d_packed", "n_words", "d_q_woff", "d_q_len",
                                                           "d_t_woff", "d_t_len", "d_q_rc", "n_pairs", "only_aligned", "d_q_row", "d_a_row",
                                                           "d_t_row", "row_cap", "d_row_off", "row_needed", "stream"]
    assert args("wfahip_alignment_text_packed") == ["r", "packed", "n_words", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "only_aligned",
                                                    "n_threads", "out"]
    assert len(_lib.lib().wfahip_alignment_text_packed_device.argtypes) == 20 and len(_lib.lib().wfahip_alignment_text_packed.argtypes) == 11
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.alignment_text_tensors_packed) == ["self", "rec", "ops", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc",
                                                                  "only_aligned", "out", "stream"]
    assert sig(wfa_amd.alignment_text_packed) == ["batch_result", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "only_aligned",
                                                  "n_threads"]
    p = inspect.signature(wfa_amd.alignment_text_packed).parameters
    assert p["n_threads"].default == 8 and p["only_aligned"].default is False and p["q_rc"].default is None
    p = inspect.signature(wfa_amd.Aligner.alignment_text_tensors_packed).parameters
    assert p["q_rc"].default is None and p["only_aligned"].default is False and p["out"].default is None and p["stream"].default is None


def test_case_set_is_what_it_claims():
    """ACGT only, the lengths of altext_cases' set, flagged queries stored as reverse complements, stale offsets where nothing
    renders, the last sequence ending exactly at the end of the words (every length 1 .. 70 at every start position is
    tests/altext_pk_host_test.cpp's)"""
    cases = P.with_acgt(A.cases())
    assert [(len(c[2]), len(c[3])) for c in cases] == [(len(c[2]), len(c[3])) for c in A.cases()]
    assert all(set(c[2] + c[3]) <= set(b"ACGT") for c in cases)
    words, q_woff, q_len, t_woff, t_len, q_rc = P.pack(cases, P.flags_of("alt", len(cases)))
    live = np.array([P.renders(c) for c in cases])
    assert (q_woff[~live] > len(words)).all() and q_rc[live].any() and not q_rc[live].all()
    assert int(max((q_woff + (q_len + 15) // 16 + 1)[live].max(), (t_woff + (t_len + 15) // 16 + 1)[live].max())) == len(words)
    i = next(k for k, c in enumerate(cases) if live[k] and q_rc[k] and len(c[2]) > 40)
    w = words[int(q_woff[i]):]
    decoded = bytes(b"ACTG"[(int(w[p // 16]) >> (2 * (p % 16))) & 3] for p in range(len(cases[i][2])))
    assert decoded == P.revcomp(cases[i][2]) != cases[i][2]
    assert P.pack_seq(b"ACGT" * 4 + b"T").tolist() == [0xB4B4B4B4, 2, 0]


@pytest.mark.parametrize("n_threads", [1, 8])
@pytest.mark.parametrize("only_aligned", [0, 1])
@pytest.mark.parametrize("flags", ["none", "all", "alt"])
def test_host_renderer_on_synthetic_cases(built, flags, only_aligned, n_threads):
    cases = P.with_acgt(A.cases())
    fl = P.flags_of(flags, len(cases))
    a = P.arrays(cases, fl)
    rc, txt = _call(a, only_aligned, n_threads)
    assert rc == 0
    _check(txt, cases, only_aligned)
    b = P.arrays(cases, fl)  # the inputs were only read
    for k in ("status", "ops_off", "ops_len", "ops"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["pk"] + a["win"], b["pk"] + b["win"]))
    if flags == "none":  # a null flag array is the array of zeros
        rc, txt = _call(a, only_aligned, n_threads, flags=False)
        assert rc == 0
        _check(txt, cases, only_aligned)


@pytest.mark.parametrize("only_aligned", [0, 1])
def test_tail_bits_and_pad_words_do_not_count(built, only_aligned):
    cases = P.with_acgt(A.cases())
    fl = P.flags_of("alt", len(cases))
    clean = P.arrays(cases, fl)
    for seed in (5, 6):
        junk = P.arrays(cases, fl, junk_tails=seed)
        assert not np.array_equal(junk["pk"][0], clean["pk"][0])
        rc, txt = _call(junk, only_aligned, 3)
        assert rc == 0
        _check(txt, cases, only_aligned)


def test_python_wrapper(built):
    import wfa_amd
    cases = P.with_acgt(A.cases())
    fl = P.flags_of("alt", len(cases))
    a = P.arrays(cases, fl)
    z = np.zeros(len(cases), np.uint32)
    qbegin, qend, tbegin, tend = a["win"]
    br = wfa_amd.BatchResult(a["status"], z, tbegin, tend, qbegin, qend, z, z, z, z, a["ops_off"], a["ops_len"], a["ops"])
    for only in (False, True):
        got = wfa_amd.alignment_text_packed(br, *a["pk"], only_aligned=only, n_threads=3)
        want = A.expected(cases, only)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert got[0].dtype == np.uint8 and got[3].dtype == np.uint64
    with pytest.raises(ValueError):
        wfa_amd.alignment_text_packed(br, *a["pk"][:5], q_rc=a["pk"][5][:3])
    with pytest.raises(ValueError):
        wfa_amd.alignment_text_packed(br, *a["pk"], n_threads=0)
    with pytest.raises(ValueError):
        wfa_amd.alignment_text_packed(br, a["pk"][0].reshape(1, -1), *a["pk"][1:])
    import torch
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    cpu = lambda shape, dt: torch.zeros(shape, dtype=dt)
    with pytest.raises(ValueError):
        al.alignment_text_tensors_packed(cpu((2, 16), torch.int32), cpu(4, torch.int64), cpu(8, torch.int32), cpu(2, torch.int64),
                                         cpu(2, torch.int32), cpu(2, torch.int64), cpu(2, torch.int32))   # on the host


def test_host_renderer_checks(built):
    """every check next to the same input at the bound: WFAHIP_ERR_BAD_ARG with out zeroed, and a pass"""
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG
    free = lambda txt: _lib.lib().wfahip_align_texts_free(C.byref(txt))

    def bad(only, a, **kw):
        rc, txt = _call(a, only, 2, **kw)
        assert rc == BAD and txt.n == 0 and txt.n_bytes == 0 and not txt.q_row and not txt.a_row and not txt.t_row and not txt.off

    def good(only, a, cols, **kw):
        rc, txt = _call(a, only, 2, **kw)
        assert rc == 0 and txt.n_bytes == cols
        free(txt)
    for flag in (0, 1):
        one = lambda **kw: P.one(flag, **kw)
        good(0, one(), 11)
        good(1, one(), 4)
        # the words: the later sequence ends exactly at n_words; one word fewer and it is outside
        n_words = len(one()["pk"][0])
        for only in (0, 1):
            good(only, one(n_words=n_words), [11, 4][only])
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
        # the pad word counts: a sequence of 16 k bases needs k + 1 words
        bad(0, one(**{last[0] + "_len": 16 * (P.packed_words(last_len) - 1) + 1}))
        # the ops consume one base more than the sequence holds (whole sequences), or than the window holds (trimmed)
        bad(0, one(q_len=6))
        bad(0, one(t_len=8))
        good(1, one(q_len=6), 4)          # (trimmed, only the window counts: query bases [1, 5) lie in 6)
        bad(1, one(qend=4))
        bad(1, one(tend=5))
        bad(1, one(tbegin=4))
        good(1, one(qbegin=1), 4)         # a window with room to spare
        # the trim checks
        bad(1, one(qbegin=0))
        bad(1, one(tbegin=0))
        bad(1, one(qbegin=-3))
        bad(1, one(qend=8))               # QEND = q_len + 1
        bad(1, one(tend=10))
        good(1, one(qbegin=4, qend=7), 4)  # ... QEND = q_len is inside
        bad(1, one(qbegin=6, qend=4))     # QBEGIN - 1 > QEND
        bad(1, one(qbegin=6, qend=5))     # QBEGIN - 1 == QEND: an empty window, too short for 4M
        good(0, one(qbegin=0, qend=-1, tbegin=77, tend=-5), 11)  # (not trimmed: the record's windows are not looked at)
        # an op range one past n_ops
        n_ops = len(a["ops"])
        bad(0, one(ops_off=n_ops - len(P.PAIR[1]) + 1))
        good(0, one(ops_off=a["ops_off"][0]), 11)
        bad(1, one(ops_len=n_ops + 1, ops_off=0))
        bad(0, one(ops_off=1 << 63))
    # the rows of the flagged pair are those of the forward one: the words hold the reverse complement, the rows the record's strand
    for flag in (0, 1):
        rc, txt = _call(P.one(flag), 1, 0)   # (n_threads <= 0 is one thread)
        assert rc == 0 and bytes(txt.q_row[:4]) == b"ACGT" and bytes(txt.a_row[:4]) == b"||||" and bytes(txt.t_row[:4]) == b"ACGT"
        free(txt)
    # the offsets of a pair that renders nothing are never looked at: not OK, no op, no column, and trimmed no M op
    for flag in (0, 1):
        cases = [P.PAIR, P.NOT_OK, P.NO_COLUMN, (P.OK, [], b"", b"", 0, 0, 0, 0), (P.OK, [P.op("X", 2), P.op("I", 1)], b"AC", b"GTA", 1, 2, 1, 3)]
        a = P.arrays(cases, [flag] * 5, seed=2)
        words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
        rc, txt = _call(a, 0, 2)
        assert rc == 0
        _check(txt, cases, 0)
        assert q_woff[1] == q_woff[3] == P.STALE_WOFF            # (pack gave the pairs without ops stale offsets)
        q_woff[2] = t_woff[2] = len(words)                        # no column: one word beyond, in both modes
        q_len[2] = t_len[2] = 1000
        rc, txt = _call(a, 0, 2)
        assert rc == 0
        _check(txt, cases, 0)
        q_woff[4] = len(words) - 1                                # no M op: ignored trimmed, refused untrimmed
        rc, txt = _call(a, 1, 2)
        assert rc == 0
        _check(txt, cases, 1)
        bad(0, a)
    # null arguments
    for name in ("status", "ops_off", "ops_len", "ops", "packed", "q_woff", "q_len", "t_woff", "t_len"):
        bad(0, P.one(), null=(name,))
    for name in ("qbegin", "qend", "tbegin", "tend"):
        bad(1, P.one(), null=(name,))
        good(0, P.one(), 11, null=(name,))
    good(0, P.one(), 11, null=("q_rc",))
    f = _lib.lib().wfahip_alignment_text_packed
    txt = _lib.AlignTexts()
    assert f(None, None, 0, None, None, None, None, None, 0, 1, C.byref(txt)) == BAD
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, None, 0, 1, None) == BAD
    # no pairs: a zeroed out whose off holds one 0
    txt.n = 99
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, None, 1, 4, C.byref(txt)) == 0
    assert txt.n == 0 and txt.n_bytes == 0 and not txt.q_row and txt.off and txt.off[0] == 0
    free(txt)
    free(txt)


def test_ops_of_wf_adaptive_that_overrun_the_sequences_are_refused(built):
    """pair 61 309 of the benchmark's 1 kbp batch, both strands: under wf-adaptive the reference's ops consume one base more than
    both sequences hold (tests/test_altext_abi.py restates it).  Untrimmed: BAD_ARG.  Trimmed the windows are the record's and the
    rows render; without wf-adaptive the same pair renders in both modes."""
    import wfa_amd
    from oracle import oracle as O
    from wfa_amd import _lib
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=3, n_pairs=3, length=1000, error_rate=0.05, first_index=61308)
    b = blob.tobytes()
    qs = [b[int(o):int(o) + int(n)] for o, n in zip(q_off, q_len)]
    ts = [b[int(o):int(o) + int(n)] for o, n in zip(t_off, t_len)]
    arrays = wfa_amd.make_blob(qs, ts)
    for adaptive, overrun in (((10, 50, 1), True), (None, False)):
        w = O.align_batch(O.make_params(global_alignment=True, adaptive=adaptive), *arrays)
        assert (w.status == 0).all()
        cases = [(0, [int(x) for x in w.pair_ops(i)], qs[i], ts[i], int(w.qbegin[i]), int(w.qend[i]), int(w.tbegin[i]), int(w.tend[i]))
                 for i in range(3)]
        used = A.consumed(cases[1][1])[1:]
        assert used == ((len(qs[1]) + 1, len(ts[1]) + 1) if overrun else (len(qs[1]), len(ts[1])))
        br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions,
                                 w.ops_off, w.ops_len, w.ops)
        for flags in ([0, 0, 0], [1, 1, 1]):
            pk = P.pack(cases, flags)
            if overrun:
                with pytest.raises(_lib.WfaHipError) as ei:
                    wfa_amd.alignment_text_packed(br, *pk)
                assert ei.value.code == _lib.ERR_BAD_ARG
            else:
                got = wfa_amd.alignment_text_packed(br, *pk)
                assert all(np.array_equal(g, x) for g, x in zip(got, A.expected(cases, 0))) and len(got[0]) > 3000
            got = wfa_amd.alignment_text_packed(br, *pk, only_aligned=True)
            assert all(np.array_equal(g, x) for g, x in zip(got, A.expected(cases, 1)))


def test_device_entry_bad_args_without_device(built):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_alignment_text_packed_device, _lib.ERR_BAD_ARG
    ctx, p = C.c_void_p(1), C.c_void_p(4096)  # (everything below returns before the context -- the address 1 -- or a buffer is dereferenced)
    need = C.c_uint64(99)
    ok = [ctx, p, p, 8, p, 8, p, p, p, p, p, 1, 0, p, p, p, 8, p, C.byref(need), None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    assert call(a0=None) == BAD
    for k in ("a1", "a17", "a6", "a7", "a8", "a9"):     # d_rec, d_row_off, the offset and length arrays
        assert call(**{k: None}) == BAD, k
    assert call(a2=None) == BAD                          # d_ops null with ops_cap > 0
    assert call(a4=None) == BAD                          # the words null with n_words > 0
    assert call(a4=None, a11=0) == BAD                   # ... whatever n_pairs is
    for k in ("a13", "a14", "a15"):                      # a null plane with row_cap > 0
        assert call(**{k: None}) == BAD, k
        assert call(**{k: None}, a11=0) == BAD, k
    assert call(a11=0xFFFFFFF1) == BAD
    assert need.value == 99
    # an empty batch without an offset array touches nothing; the flags may be null
    assert call(a1=None, a2=None, a3=0, a4=None, a5=0, a6=None, a7=None, a8=None, a9=None, a10=None, a11=0, a13=None, a14=None, a15=None,
                a16=0, a17=None) == 0 and need.value == 0
    assert call(a11=0, a17=None, a18=None, a10=None) == 0


def test_decoding_rule_under_sanitizers():
    src = os.path.join(ROOT, "tests", "altext_pk_host_test.cpp")
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    for name, flags in (("altext_pk_host_test", []),
                        ("altext_pk_host_test_asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(ROOT, "build", name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "altext packed host test ok" in r.stdout
