"""CPU: CIGAR text (include/wfa_hip.h: wfahip_cigar_text_device, wfahip_cigar_text, wfahip_align_batch_text).  The entries' declarations
and bindings; the host renderer wfahip_cigar_text -- the same header functions as the kernels -- against AlignmentResult.CIGAR on
synthetic arrays (tests/cigar_cases.py) and against the oracle's own strings on aligned pairs; the argument checks the three
entries make before a context or a device is touched; and the rendering rule as a stand-alone program under the host sanitizers
(tests/cigar_host_test.cpp)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cigar_cases as K  # noqa: E402


def _results(status, ops_off, ops_len, ops):
    from wfa_amd import _lib
    r = _lib.Results()
    r.n, r.n_ops = len(status), len(ops)
    r.status = status.ctypes.data_as(C.POINTER(C.c_int32))
    r.ops_off = ops_off.ctypes.data_as(C.POINTER(C.c_uint64))
    r.ops_len = ops_len.ctypes.data_as(C.POINTER(C.c_uint32))
    r.ops = ops.ctypes.data_as(C.POINTER(C.c_uint64))
    return r


def test_entries_declared_exported_and_bound(built):
    import inspect
    import wfa_amd
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in ("wfahip_cigar_text_device", "wfahip_cigar_text", "wfahip_cigars_free", "wfahip_align_batch_text"):
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_cigar_text_device") == ["ctx", "d_rec", "d_ops", "ops_cap", "n_pairs", "only_aligned", "d_text", "text_cap",
                                                "d_text_off", "text_needed", "stream"]
    assert args("wfahip_cigar_text") == ["r", "only_aligned", "n_threads", "out"]
    assert args("wfahip_cigars_free") == ["c"]
    assert args("wfahip_align_batch_text") == ["ctx", "p", "seq_blob", "blob_bytes", "q_off", "q_len", "t_off", "t_len", "n_pairs",
                                               "only_aligned", "out", "cig"]
    assert re.search(r"typedef struct \{ uint64_t n; uint64_t n_bytes; char \*text; uint64_t \*off;\s*\} wfahip_cigars;", hdr)
    assert _lib.lib().wfahip_version() == 400
    assert [f[0] for f in _lib.Cigars._fields_] == ["n", "n_bytes", "text", "off"]
    # the Python mirror
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.align_tensors) == ["self", "blob", "q_off", "q_len", "t_off", "t_len", "max_score", "stream"]
    assert sig(wfa_amd.Aligner.cigar_tensors) == ["self", "rec", "ops", "only_aligned", "out", "stream"]
    assert sig(wfa_amd.Aligner.align_arrays_text) == ["self", "blob", "q_off", "q_len", "t_off", "t_len", "only_aligned"]
    assert sig(wfa_amd.cigar_text) == ["batch_result", "only_aligned", "n_threads"]
    assert inspect.signature(wfa_amd.cigar_text).parameters["n_threads"].default == 8
    # the kernels' unit is part of the library's build
    assert re.search(r"^UNITS\s*:=.*\bwfa_cigar\b", open(os.path.join(ROOT, "Makefile")).read(), flags=re.M)


@pytest.mark.parametrize("n_threads", [1, 3, 64])
@pytest.mark.parametrize("only_aligned", [0, 1])
def test_host_renderer_on_synthetic_arrays(built, only_aligned, n_threads):
    """digit boundaries, every letter, the trim cases, empty and failed pairs; ops out of pair order with junk between them"""
    from wfa_amd import _lib
    cases = K.base_cases() + K.seam_cases()
    assert n_threads == 64 and n_threads > len(cases) or n_threads < len(cases)
    status, ops_off, ops_len, ops = K.lay_out(cases, seed=11)
    want_text, want_off = K.expected(cases, only_aligned)
    cig = _lib.Cigars()
    assert _lib.lib().wfahip_cigar_text(C.byref(_results(status, ops_off, ops_len, ops)), only_aligned, n_threads, C.byref(cig)) == 0
    try:
        n = len(cases)
        assert cig.n == n and cig.off[0] == 0 and cig.off[n] == cig.n_bytes == len(want_text)
        got_off = np.ctypeslib.as_array(cig.off, shape=(n + 1,))
        got_text = np.ctypeslib.as_array(cig.text, shape=(int(cig.n_bytes),))
        assert np.array_equal(got_off, want_off)
        assert got_text.tobytes() == want_text.tobytes()
    finally:
        _lib.lib().wfahip_cigars_free(C.byref(cig))
    assert cig.n == 0 and cig.n_bytes == 0 and not cig.text and not cig.off
    # the inputs were only read
    s2, o2, l2, w2 = K.lay_out(cases, seed=11)
    assert np.array_equal(status, s2) and np.array_equal(ops_off, o2) and np.array_equal(ops_len, l2) and np.array_equal(ops, w2)


def test_host_renderer_per_pair_strings(built):
    """the Python wrapper, pair by pair: the rule's corner cases spelled out"""
    import wfa_amd
    cases = [(K.OK, [K.op("M", 0), K.op("~", 4294967295), K.op("M", 1000000000)]), (K.OK, [K.op("X", 1)]), (K.OK, []),
             (K.OK, [K.op("I", 2), K.op("M", 10), K.op("D", 1)]), (K.EMPTY, None), (K.OK, [K.op("M", 999999999)])]
    status, ops_off, ops_len, ops = K.lay_out(cases, seed=3)
    br = wfa_amd.BatchResult(status, *([np.zeros(len(cases), np.uint32)] * 9), ops_off, ops_len, ops)
    for only, want in ((False, [b"0M4294967295~1000000000M", b"1X", b"", b"2I10M1D", b"", b"999999999M"]),
                       (True, [b"0M4294967295~1000000000M", b"", b"", b"10M", b"", b"999999999M"])):
        text, off = wfa_amd.cigar_text(br, only_aligned=only, n_threads=2)
        assert text.dtype == np.uint8 and off.dtype == np.uint64 and off[0] == 0 and off[-1] == len(text)
        assert [text[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(cases))] == want


def test_host_renderer_empty_batch_and_empty_text(built):
    from wfa_amd import _lib
    f = _lib.lib().wfahip_cigar_text
    r, cig = _lib.Results(), _lib.Cigars()
    cig.n = cig.n_bytes = 99
    assert f(C.byref(r), 0, 4, C.byref(cig)) == 0                       # n == 0: a zeroed out whose off holds one 0
    assert cig.n == 0 and cig.n_bytes == 0 and not cig.text and cig.off and cig.off[0] == 0
    _lib.lib().wfahip_cigars_free(C.byref(cig))
    status, ops_off, ops_len, ops = K.lay_out([(K.EMPTY, None), (K.OK, []), (K.OK, [K.op("X", 1)])], seed=1)
    assert f(C.byref(_results(status, ops_off, ops_len, ops)), 1, 2, C.byref(cig)) == 0
    assert cig.n == 3 and cig.n_bytes == 0 and not cig.text and [cig.off[i] for i in range(4)] == [0, 0, 0, 0]
    _lib.lib().wfahip_cigars_free(C.byref(cig))
    _lib.lib().wfahip_cigars_free(C.byref(cig))                         # (a freed one again, and NULL: nothing happens)
    _lib.lib().wfahip_cigars_free(None)


def test_host_renderer_bad_args(built):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_cigar_text, _lib.ERR_BAD_ARG
    status, ops_off, ops_len, ops = K.lay_out([(K.OK, [K.op("M", 4), K.op("X", 1)]), (K.EMPTY, None)], seed=1, junk=False)
    cig = _lib.Cigars()
    assert f(None, 0, 1, C.byref(cig)) == BAD
    assert f(C.byref(_results(status, ops_off, ops_len, ops)), 0, 1, None) == BAD
    for null in ("status", "ops_off", "ops_len", "ops"):
        r = _results(status, ops_off, ops_len, ops)
        setattr(r, null, None)
        cig.n = 99
        assert f(C.byref(r), 0, 1, C.byref(cig)) == BAD, null
        assert cig.n == 0 and not cig.text and not cig.off
    for off, ln in ((1, 2), (3, 0), (1 << 63, 2), ((1 << 64) - 1, 2), (0, 3), (0, 0xFFFFFFFF)):  # an OK pair's ops outside [0, n_ops)
        o, l = ops_off.copy(), ops_len.copy()
        o[0], l[0] = off, ln
        assert f(C.byref(_results(status, o, l, ops)), 0, 3, C.byref(cig)) == BAD, (off, ln)
        assert not cig.text and not cig.off
    o, l = ops_off.copy(), ops_len.copy()
    o[0], l[0] = 2, 0                                                                             # an empty range at the very end is inside
    assert f(C.byref(_results(status, o, l, ops)), 0, 1, C.byref(cig)) == 0 and cig.n_bytes == 0
    _lib.lib().wfahip_cigars_free(C.byref(cig))
    assert f(C.byref(_results(status, ops_off, ops_len, ops)), 0, 0, C.byref(cig)) == 0 and cig.n_bytes == 4   # n_threads <= 0: one thread
    _lib.lib().wfahip_cigars_free(C.byref(cig))


def _pin_pairs():
    """about 200 seeded pairs of 20 to 300 bases: global, and semi-global with the target or the query overhanging"""
    rng = np.random.default_rng(2024)
    letters = np.frombuffer(b"ACGT", np.uint8)

    def mutate(s, rate):
        out = bytearray()
        for b in s:
            u = rng.random()
            if u < rate / 3:
                continue
            if u < 2 * rate / 3:
                out.append(int(rng.choice(letters)))
            if u < rate:
                out.append(int(rng.choice(letters)))
            else:
                out.append(b)
        return bytes(out) or b"A"
    pairs = []
    for k in range(200):
        n = int(rng.integers(20, 301))
        q = bytes(rng.choice(letters, n))
        t = mutate(q, [0.02, 0.05, 0.15][k % 3])
        if k % 4 == 1:
            t = bytes(rng.choice(letters, int(rng.integers(1, 40)))) + t + bytes(rng.choice(letters, int(rng.integers(1, 40))))
        elif k % 4 == 3:
            q = bytes(rng.choice(letters, int(rng.integers(1, 25)))) + q + bytes(rng.choice(letters, int(rng.integers(1, 25))))
        pairs.append((q, t, k % 4 == 0 or k % 4 == 2))
    pairs += [(b"A", b"C", True), (b"A", b"C", False), (b"ACGT", b"ACGT", True)]
    return pairs


@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 3, 1)])
def test_independent_pin_against_the_oracle(built, known_answers, pen):
    """the oracle aligns on the CPU; its ops through wfahip_cigar_text must give the oracle's own cigar and cigar_trimmed, and the
    published string where the fixture pins it"""
    import wfa_amd
    from oracle import oracle as O
    jobs = [(q, t, O.make_params(*pen, global_alignment=g), None) for q, t, g in _pin_pairs()]
    if pen == (4, 6, 2):
        for ka in known_answers["vectors"]:
            prm = O.make_params(global_alignment=ka["mode"] == "global", adaptive=tuple(ka["adaptive"]) if ka.get("adaptive") else None)
            jobs.append((ka["q"].encode(), ka["t"].encode(), prm, ka))
    results, aligners = [], {}
    for q, t, prm, ka in jobs:
        key = bytes(prm)
        if key not in aligners:
            aligners[key] = O.Aligner(prm)
        r = aligners[key].align(q, t)
        assert r.status == O.OK
        results.append(r)
    cases = [(K.OK, r.ops) for r in results]
    status, ops_off, ops_len, ops = K.lay_out(cases, seed=9)
    br = wfa_amd.BatchResult(status, *([np.zeros(len(cases), np.uint32)] * 9), ops_off, ops_len, ops)
    n_exact = 0
    for only in (False, True):
        text, off = wfa_amd.cigar_text(br, only_aligned=only, n_threads=5)
        for i, (r, job) in enumerate(zip(results, jobs)):
            got = text[int(off[i]):int(off[i + 1])].tobytes().decode()
            assert got == (r.cigar_trimmed() if only else r.cigar), i
            if job[3] is not None and job[3].get("cigar_exact") and not only:
                assert got == job[3]["cigar"], job[3]["id"]
                n_exact += 1
    assert pen != (4, 6, 2) or n_exact >= 1
    assert any(r.cigar != r.cigar_trimmed() for r in results) and any(r.cigar_trimmed() == "" for r in results)


def test_device_entry_bad_args_without_device(built):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_cigar_text_device, _lib.ERR_BAD_ARG
    ctx, p = C.c_void_p(1), C.c_void_p(4096)  # (everything below returns before the context -- the address 1 -- or a buffer is dereferenced)
    need = C.c_uint64(99)
    assert f(None, p, p, 8, 1, 0, p, 8, p, C.byref(need), None) == BAD
    assert f(ctx, None, p, 8, 1, 0, p, 8, p, C.byref(need), None) == BAD       # d_rec
    assert f(ctx, p, p, 8, 1, 0, p, 8, None, C.byref(need), None) == BAD       # d_text_off
    assert f(ctx, p, None, 8, 1, 0, p, 8, p, C.byref(need), None) == BAD       # d_ops null with ops_cap > 0
    assert f(ctx, p, p, 8, 1, 0, None, 8, p, C.byref(need), None) == BAD       # d_text null with text_cap > 0
    assert f(ctx, p, None, 8, 0, 0, None, 0, None, C.byref(need), None) == BAD  # ... whatever n_pairs is
    assert f(ctx, None, None, 0, 0, 0, None, 8, None, C.byref(need), None) == BAD
    assert need.value == 99
    # an empty batch without an offset array touches nothing
    assert f(ctx, None, None, 0, 0, 0, None, 0, None, C.byref(need), None) == 0 and need.value == 0
    assert f(ctx, None, None, 0, 0, 1, None, 0, None, None, None) == 0


def test_align_batch_text_bad_args_without_device(built):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_align_batch_text, _lib.ERR_BAD_ARG
    prm = _lib.Params(4, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    blob = (C.c_uint8 * 8)(*b"ACGTACGT")
    off0, off4, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(4), (C.c_uint32 * 1)(4)
    ctx = C.c_void_p(1)
    out, cig = _lib.Results(), _lib.Cigars()
    ok = lambda: (ctx, C.byref(prm), blob, 8, off0, ln, off4, ln, 1, 0, C.byref(out), C.byref(cig))

    def call(**kw):
        a = list(ok())
        for k, v in kw.items():
            a[int(k[1:])] = v
        out.n, cig.n = 99, 99
        return f(*a)
    assert call(a0=None) == BAD
    assert call(a10=None) == BAD and cig.n == 0
    assert call(a11=None) == BAD
    assert call(a1=None) == BAD and out.n == 0 and cig.n == 0
    assert call(a2=None) == BAD
    for k in ("a4", "a5", "a6", "a7"):
        assert call(**{k: None}) == BAD, k
    assert call(a4=(C.c_uint64 * 1)(5)) == BAD              # a query of 4 bases at 5 of an 8-byte blob
    assert call(a6=(C.c_uint64 * 1)(1 << 63)) == BAD
    assert call(a7=(C.c_uint32 * 1)(5)) == BAD
    bad = _lib.Params(0, 6, 2, 1, 0, (0, 0), 0, 0, 0)
    assert call(a1=C.byref(bad)) == _lib.ERR_UNSUPPORTED
    # an empty batch is fine without a device: zeroed results, no text, one offset
    assert call(a2=None, a3=0, a4=None, a5=None, a6=None, a7=None, a8=0) == 0
    assert out.n == 0 and not out.status and not out.ops and cig.n == 0 and cig.n_bytes == 0 and not cig.text and cig.off[0] == 0
    _lib.lib().wfahip_cigars_free(C.byref(cig))
    _lib.lib().wfahip_results_free(C.byref(out))


def test_python_wrappers_refuse_wrong_shapes_before_the_call(built):
    import torch
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    blob = np.frombuffer(b"ACGTACGT", np.uint8)
    off, ln = np.array([0, 4], np.uint64), np.array([4, 4], np.uint32)
    with pytest.raises(ValueError):
        al.align_arrays_text(blob, off, ln, off[:1], ln)
    with pytest.raises(ValueError):
        al.align_arrays_text(blob, off, ln, off, ln[:1])
    with pytest.raises(ValueError):
        al.align_arrays_text(blob.reshape(2, 4), off, ln, off, ln)
    with pytest.raises(ValueError):
        al.align_tensors(blob, off, ln, off, ln)                                  # numpy arrays
    cpu = lambda a, dt: torch.from_numpy(a.astype(dt))
    with pytest.raises(ValueError):
        al.align_tensors(cpu(blob, np.uint8), cpu(off, np.int64), cpu(ln, np.int32), cpu(off, np.int64), cpu(ln, np.int32))  # on the host
    with pytest.raises(ValueError):
        al.cigar_tensors(np.zeros((2, 16), np.int32), np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        al.cigar_tensors(torch.zeros((2, 16), dtype=torch.int32), torch.zeros(4, dtype=torch.int64))                        # on the host
    br = wfa_amd.BatchResult(np.zeros(2, np.int32), *([np.zeros(2, np.uint32)] * 9), np.zeros(3, np.uint64), np.zeros(2, np.uint32),
                             np.zeros(0, np.uint64))
    with pytest.raises(ValueError):
        wfa_amd.cigar_text(br)                                                    # ops_off of another length
    br.ops_off = np.zeros(2, np.uint64)
    with pytest.raises(ValueError):
        wfa_amd.cigar_text(br, n_threads=0)
    text, off = wfa_amd.cigar_text(br)
    assert len(text) == 0 and list(off) == [0, 0, 0]


def test_rendering_rule_under_sanitizers():
    exe = os.path.join(ROOT, "build", "cigar_host_test_asan_ubsan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cigar_host_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cigar host test ok" in r.stdout
