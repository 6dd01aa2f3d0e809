"""CPU: the display rows (include/wfa_hip.h: wfahip_alignment_text_device, wfahip_alignment_text).  The entries' declarations and
bindings; the host renderer wfahip_alignment_text -- the same header functions as the kernels -- against
AlignmentResult.AlignmentText on synthetic records, ops and sequences (tests/altext_cases.py), on the oracle's own alignments and on
the published three-line texts; every check that stands where the reference would index out of range; the argument checks the
entries make before a context or a device is touched; and the rendering rule as a stand-alone program under the host sanitizers
(tests/altext_host_test.cpp)."""
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
import cigar_cases as K  # noqa: E402


def _call(a, only, n_threads, blob_bytes=None, null=()):
    """wfahip_alignment_text on _arrays' dict: (return code, the struct -- the caller frees it)"""
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
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    vp = lambda name, x: None if name in null else x.ctypes.data_as(C.c_void_p)
    txt = _lib.AlignTexts()
    txt.n = txt.n_bytes = 99
    rc = _lib.lib().wfahip_alignment_text(C.byref(r), vp("blob", blob), len(blob) if blob_bytes is None else blob_bytes, vp("q_off", q_off),
                                          vp("q_len", q_len), vp("t_off", t_off), vp("t_len", t_len), only, n_threads, C.byref(txt))
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
    for name in ("wfahip_alignment_text_device", "wfahip_alignment_text", "wfahip_align_texts_free"):
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_alignment_text_device") == ["ctx", "d_rec", "d_ops", "ops_cap", "d_seq_blob", "blob_bytes", "d_q_off", "d_q_len",
                                                    "d_t_off", "d_t_len", "n_pairs", "only_aligned", "d_q_row", "d_a_row", "d_t_row",
                                                    "row_cap", "d_row_off", "row_needed", "stream"]
    assert args("wfahip_alignment_text") == ["r", "seq_blob", "blob_bytes", "q_off", "q_len", "t_off", "t_len", "only_aligned", "n_threads",
                                             "out"]
    assert args("wfahip_align_texts_free") == ["t"]
    assert re.search(r"typedef struct \{ uint64_t n, n_bytes; char \*q_row, \*a_row, \*t_row; uint64_t \*off;\s*\} wfahip_align_texts;", hdr)
    assert len(_lib.lib().wfahip_alignment_text_device.argtypes) == 19 and len(_lib.lib().wfahip_alignment_text.argtypes) == 10
    assert [f[0] for f in _lib.AlignTexts._fields_] == ["n", "n_bytes", "q_row", "a_row", "t_row", "off"]
    assert C.sizeof(_lib.AlignTexts) == 48
    assert _lib.lib().wfahip_version() == 400
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.alignment_text_tensors) == ["self", "rec", "ops", "blob", "q_off", "q_len", "t_off", "t_len", "only_aligned",
                                                           "out", "stream"]
    assert sig(wfa_amd.alignment_text) == ["batch_result", "blob", "q_off", "q_len", "t_off", "t_len", "only_aligned", "n_threads"]
    p = inspect.signature(wfa_amd.alignment_text).parameters
    assert p["n_threads"].default == 8 and p["only_aligned"].default is False
    p = inspect.signature(wfa_amd.Aligner.alignment_text_tensors).parameters
    assert p["only_aligned"].default is False and p["out"].default is None and p["stream"].default is None


def test_case_set_is_what_it_claims():
    """the synthetic set: every byte value in the sequences, every residue mod 16 among the offsets, rows starting at every byte
    alignment, and trimmed windows that are NOT where the trimmed-away ops end"""
    cases = A.cases()
    blob, q_off, q_len, t_off, t_len = A.blob(cases)
    live = np.array([c[0] == A.OK and bool(c[1]) for c in cases])
    assert set(np.unique(blob)) == set(range(256))
    assert set(int(o) % 16 for o in np.concatenate([q_off[live], t_off[live]])) == set(range(16))
    assert (q_off[~live] > len(blob)).all()
    for only in (0, 1):
        off = A.expected(cases, only)[3]
        assert set(int(o) % 4 for o in off[:-1][np.diff(off.astype(np.int64)) > 0]) == {0, 1, 2, 3}
    moved = 0
    for st, ops, q, t, qbegin, qend, tbegin, tend in cases:
        if st == A.OK and ops and A.trim(ops)[1]:
            _, pq, pt = A.consumed(ops[:A.trim(ops)[0]])
            moved += qbegin != pq + 1 and tbegin != pt + 1
    assert moved >= 8
    assert max(len(c[1] or []) for c in cases) == 200 and any(A.consumed(c[1] or [])[0] >= 70000 for c in cases)


@pytest.mark.parametrize("n_threads", [1, 3, 64])
@pytest.mark.parametrize("only_aligned", [0, 1])
def test_host_renderer_on_synthetic_cases(built, only_aligned, n_threads):
    cases = A.cases()
    assert n_threads == 64 and n_threads > len(cases) or n_threads < len(cases)
    a = A.arrays(cases)
    rc, txt = _call(a, only_aligned, n_threads)
    assert rc == 0
    _check(txt, cases, only_aligned)
    b = A.arrays(cases)  # the inputs were only read
    for k in ("status", "ops_off", "ops_len", "ops"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["seqs"] + a["win"], b["seqs"] + b["win"]))


def _oracle_cases(pairs, prm):
    from oracle import oracle as O
    al = O.Aligner(prm)
    out = []
    for q, t in pairs:
        r = al.align(q, t)
        out.append((int(r.status), list(r.ops) if r.status == O.OK else None, q, t, r.qbegin, r.qend, r.tbegin, r.tend))
    return out


@pytest.mark.parametrize("glob", [True, False])
def test_host_renderer_on_the_oracles_alignments(built, glob):
    """200 seeded pairs -- semi-global with the targets overhanging on both sides -- + an empty pair, a pair with an N, A against C:
    the oracle aligns, its results go through wfahip_alignment_text via the Python wrapper, AlignmentText pair by pair is the
    reference"""
    import wfa_amd
    from oracle import oracle as O
    rng = np.random.default_rng(31 + glob)
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=41 + glob, n_pairs=200, length=120, error_rate=0.08)
    b = blob.tobytes()
    qs = [b[int(o):int(o) + int(n)] for o, n in zip(q_off, q_len)]
    ts = [b[int(o):int(o) + int(n)] for o, n in zip(t_off, t_len)]
    if not glob:
        rnd = lambda k: bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))
        ts = [rnd(int(rng.integers(1, 40))) + t + rnd(int(rng.integers(1, 40))) for t in ts]
    qs += [b"", b"ACGTNACGTTGCA", b"A"]
    ts += [b"ACGT", b"ACGTAACGTTGCA", b"C"]
    arrays = wfa_amd.make_blob(qs, ts)
    w = O.align_batch(O.make_params(global_alignment=glob, adaptive=(10, 50, 1)), *arrays, n_threads=4)
    assert list(w.status[-3:]) == [1, 0, 0] and (w.status[:-3] == 0).all()
    br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions,
                             w.ops_off, w.ops_len, w.ops)
    n_trimmed_away = 0
    for only in (False, True):
        q_row, a_row, t_row, off = wfa_amd.alignment_text(br, *arrays, only_aligned=only, n_threads=5)
        assert q_row.dtype == a_row.dtype == t_row.dtype == np.uint8 and off.dtype == np.uint64
        assert off[0] == 0 and off[-1] == len(q_row) == len(a_row) == len(t_row)
        for i in range(len(qs)):
            if w.status[i] != 0:
                want = (b"", b"", b"")
            else:
                case = (0, [int(x) for x in w.pair_ops(i)], qs[i], ts[i], int(w.qbegin[i]), int(w.qend[i]), int(w.tbegin[i]), int(w.tend[i]))
                want = A.rows_of(case, only)
            s = slice(int(off[i]), int(off[i + 1]))
            assert (q_row[s].tobytes(), a_row[s].tobytes(), t_row[s].tobytes()) == want, (i, only)
            n_trimmed_away += only and len(want[0]) < len(A.rows_of(case, False)[0]) if w.status[i] == 0 else 0
        if only:
            assert off[-1] == off[-2]  # A against C, trimmed: empty rows
    assert glob or n_trimmed_away > 100


def test_host_renderer_on_the_published_texts(built, known_answers):
    """the three-line texts of the fixture that test_oracle_golden.py::test_alignment_text renders with AlignmentText"""
    from oracle import oracle as O
    cases, texts = [], []
    for ka in known_answers["vectors"]:
        if "text" not in ka:
            continue
        prm = O.make_params(global_alignment=ka["mode"] == "global", adaptive=tuple(ka["adaptive"]) if ka.get("adaptive") else None)
        cases += _oracle_cases([(ka["q"].encode(), ka["t"].encode())], prm)
        texts.append(ka["text"])
    assert len(cases) >= 3
    rc, txt = _call(A.arrays(cases), 0, 2)
    assert rc == 0
    for i, text in enumerate(texts):
        rows = [bytes(p[int(txt.off[i]):int(txt.off[i + 1])]).decode() for p in (txt.q_row, txt.a_row, txt.t_row)]
        assert rows[0] == text[0] and rows[1].rstrip() == text[1].rstrip() and rows[2] == text[2]
    _check(txt, cases, 0)
    rc, txt = _call(A.arrays(cases), 1, 2)
    assert rc == 0
    _check(txt, cases, 1)


def test_host_renderer_checks(built):
    """where the reference would index out of range the call is WFAHIP_ERR_BAD_ARG with out zeroed; at the bound it passes"""
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
    good(0, A.one(), 11)
    good(1, A.one(), 4)
    # the ops consume one base more than the sequence holds (whole sequences), or than the window holds (trimmed)
    bad(0, A.one(q_len=6))
    bad(0, A.one(t_len=8))
    good(1, A.one(q_len=6), 4)      # (trimmed, only the window counts: query bytes [1, 5) lie in 6)
    bad(1, A.one(qend=4))
    bad(1, A.one(tend=5))
    bad(1, A.one(tbegin=4))
    good(1, A.one(qbegin=1), 4)     # a window with room to spare
    # the windows themselves
    bad(1, A.one(qbegin=0))
    bad(1, A.one(tbegin=0))
    bad(1, A.one(qbegin=-3))
    bad(1, A.one(qend=8))           # QEND = q_len + 1
    bad(1, A.one(tend=10))
    good(1, A.one(qbegin=4, qend=7), 4)   # ... QEND = q_len is inside
    bad(1, A.one(qbegin=6, qend=4))  # QBEGIN - 1 > QEND
    bad(1, A.one(qbegin=6, qend=5))  # QBEGIN - 1 == QEND: an empty window, too short for 4M
    good(0, A.one(qbegin=0, qend=-1, tbegin=77, tend=-5), 11)  # (not trimmed: the record's windows are not looked at)
    # a sequence one byte outside the blob
    a = A.one()
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    last = "q_off" if q_off[0] > t_off[0] else "t_off"
    end = int(max(q_off[0] + q_len[0], t_off[0] + t_len[0]))
    for only in (0, 1):
        bad(only, a, blob_bytes=end - 1)
        good(only, a, [11, 4][only], blob_bytes=end)
        bad(only, A.one(**{last: len(blob) - [6, 8][last == "t_off"]}))
        bad(only, A.one(**{last: 1 << 63}))
        bad(only, A.one(**{last: (1 << 64) - 1}))
    # an op range one past n_ops
    n_ops = len(a["ops"])
    bad(0, A.one(ops_off=n_ops - len(A.PAIR[1]) + 1))
    good(0, A.one(ops_off=a["ops_off"][0]), 11)
    bad(1, A.one(ops_len=n_ops + 1, ops_off=0))
    bad(0, A.one(ops_off=1 << 63))
    # null arguments
    for name in ("status", "ops_off", "ops_len", "ops", "blob", "q_off", "q_len", "t_off", "t_len"):
        bad(0, A.one(), null=(name,))
    for name in ("qbegin", "qend", "tbegin", "tend"):
        bad(1, A.one(), null=(name,))
        good(0, A.one(), 11, null=(name,))
    f = _lib.lib().wfahip_alignment_text
    txt = _lib.AlignTexts()
    assert f(None, None, 0, None, None, None, None, 0, 1, C.byref(txt)) == BAD
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, 0, 1, None) == BAD
    # no pairs: a zeroed out whose off holds one 0; n_threads <= 0 is one thread
    txt.n = 99
    assert f(C.byref(_lib.Results()), None, 0, None, None, None, None, 1, 4, C.byref(txt)) == 0
    assert txt.n == 0 and txt.n_bytes == 0 and not txt.q_row and txt.off and txt.off[0] == 0
    free(txt)
    free(txt)
    _lib.lib().wfahip_align_texts_free(None)
    good(0, A.one(), 11)
    rc, txt = _call(A.one(), 1, 0)
    assert rc == 0 and bytes(txt.q_row[:4]) == b"ACGT" and bytes(txt.a_row[:4]) == b"||||" and bytes(txt.t_row[:4]) == b"ACGT"
    free(txt)


def test_ops_of_wf_adaptive_that_overrun_the_sequences_are_refused(built):
    """pair 61 309 of the benchmark's 1 kbp batch: under wf-adaptive the reference's ops end ..5M1X3I and consume 1 001 and 1 007
    bases of 1 000 and 1 006 (the oracle restates it).  Untrimmed the reference would index out of range: BAD_ARG.  Trimmed the
    windows are the record's and the rows render; without wf-adaptive the same pair renders in both modes."""
    import wfa_amd
    from oracle import oracle as O
    from wfa_amd import _lib
    arrays = wfa_amd.generate_pairs(seed=3, n_pairs=3, length=1000, error_rate=0.05, first_index=61308)
    for adaptive, overrun in (((10, 50, 1), True), (None, False)):
        w = O.align_batch(O.make_params(global_alignment=True, adaptive=adaptive), *arrays)
        assert (w.status == 0).all()
        used = [A.consumed([int(x) for x in w.pair_ops(i)])[1:] for i in range(3)]
        lens = [(int(arrays[2][i]), int(arrays[4][i])) for i in range(3)]
        assert used[0] == lens[0] and used[2] == lens[2]
        assert used[1] == ((lens[1][0] + 1, lens[1][1] + 1) if overrun else lens[1])
        br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions,
                                 w.ops_off, w.ops_len, w.ops)
        if overrun:
            with pytest.raises(_lib.WfaHipError) as ei:
                wfa_amd.alignment_text(br, *arrays)
            assert ei.value.code == _lib.ERR_BAD_ARG
        else:
            assert len(wfa_amd.alignment_text(br, *arrays)[0]) > 3000
        q_row, a_row, t_row, off = wfa_amd.alignment_text(br, *arrays, only_aligned=True)
        for i in range(3):
            case = (0, [int(x) for x in w.pair_ops(i)], *_seq(arrays, i), int(w.qbegin[i]), int(w.qend[i]), int(w.tbegin[i]), int(w.tend[i]))
            s = slice(int(off[i]), int(off[i + 1]))
            assert (q_row[s].tobytes(), a_row[s].tobytes(), t_row[s].tobytes()) == A.rows_of(case, True)


def _seq(arrays, i):
    blob, q_off, q_len, t_off, t_len = arrays
    b = blob.tobytes()
    return b[int(q_off[i]):int(q_off[i]) + int(q_len[i])], b[int(t_off[i]):int(t_off[i]) + int(t_len[i])]


def test_device_entry_bad_args_without_device(built):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_alignment_text_device, _lib.ERR_BAD_ARG
    ctx, p = C.c_void_p(1), C.c_void_p(4096)  # (everything below returns before the context -- the address 1 -- or a buffer is dereferenced)
    need = C.c_uint64(99)
    ok = [ctx, p, p, 8, p, 8, p, p, p, p, 1, 0, p, p, p, 8, p, C.byref(need), None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    assert call(a0=None) == BAD
    for k in ("a1", "a16", "a6", "a7", "a8", "a9"):     # d_rec, d_row_off, the offset and length arrays
        assert call(**{k: None}) == BAD, k
    assert call(a2=None) == BAD                          # d_ops null with ops_cap > 0
    assert call(a4=None) == BAD                          # the blob null with blob_bytes > 0
    for k in ("a12", "a13", "a14"):                      # a null plane with row_cap > 0
        assert call(**{k: None}) == BAD, k
        assert call(**{k: None}, a10=0) == BAD, k        # ... whatever n_pairs is
    assert call(a10=0xFFFFFFF1) == BAD
    assert need.value == 99
    # an empty batch without an offset array touches nothing
    assert call(a1=None, a2=None, a3=0, a4=None, a5=0, a6=None, a7=None, a8=None, a9=None, a10=0, a12=None, a13=None, a14=None, a15=0,
                a16=None) == 0 and need.value == 0
    assert call(a10=0, a16=None, a17=None) == 0


def test_python_wrappers_refuse_wrong_shapes_before_the_call(built):
    import torch
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    cpu = lambda shape, dt: torch.zeros(shape, dtype=dt)
    good = (cpu((2, 16), torch.int32), cpu(4, torch.int64), cpu(8, torch.uint8), cpu(2, torch.int64), cpu(2, torch.int32),
            cpu(2, torch.int64), cpu(2, torch.int32))
    with pytest.raises(ValueError):
        al.alignment_text_tensors(*good)                                            # on the host
    with pytest.raises(ValueError):
        al.alignment_text_tensors(np.zeros((2, 16), np.int32), *good[1:])           # numpy arrays
    n = 2
    z = lambda dt: np.zeros(n, dt)
    br = wfa_amd.BatchResult(z(np.int32), *([z(np.uint32)] * 9), z(np.uint64), z(np.uint32), np.zeros(0, np.uint64))
    seqs = (np.frombuffer(b"ACGTACGT", np.uint8), z(np.uint64), z(np.uint32), z(np.uint64), z(np.uint32))
    rows = wfa_amd.alignment_text(br, *seqs)
    assert [len(r) for r in rows] == [0, 0, 0, 3] and list(rows[3]) == [0, 0, 0]
    with pytest.raises(ValueError):
        wfa_amd.alignment_text(br, *seqs, n_threads=0)
    with pytest.raises(ValueError):
        wfa_amd.alignment_text(br, seqs[0], seqs[1][:1], *seqs[2:])
    with pytest.raises(ValueError):
        wfa_amd.alignment_text(br, seqs[0].reshape(2, 4), *seqs[1:])
    br.qend = np.zeros(3, np.int32)
    with pytest.raises(ValueError):
        wfa_amd.alignment_text(br, *seqs)
    br.qend = np.zeros(2, np.int32)
    br.status = np.array([0, 1], np.int32)
    br.ops_len = np.array([1, 0], np.uint32)                                        # an op range outside the (empty) ops
    with pytest.raises(wfa_amd.aligner.L.WfaHipError) as ei:
        wfa_amd.alignment_text(br, *seqs)
    assert ei.value.code == wfa_amd.aligner.L.ERR_BAD_ARG


def test_rendering_rule_under_sanitizers():
    src = os.path.join(ROOT, "tests", "altext_host_test.cpp")
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    for name, flags in (("altext_host_test", []), ("altext_host_test_asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(ROOT, "build", name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "altext host test ok" in r.stdout
