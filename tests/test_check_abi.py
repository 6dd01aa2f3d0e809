"""CPU: the check (include/wfa_hip.h: wfahip_check_alignments_device, _packed_device, wfahip_check_alignments, _packed).  The
entries' declarations and bindings; the host entries -- the same header functions as the kernels -- against the restatement of the
rule in tests/check_cases.py, on a synthetic set and on the oracle's own alignments, flag for flag; the argument checks made before a
context or a device is touched; and the rule as a stand-alone program under the host sanitizers (tests/check_host_test.cpp)."""
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
import check_cases as X  # noqa: E402
import check_batches as B  # noqa: E402


def _host(a, prm, packed=False, mask=X.ALL, n_threads=8):
    """the Python wrapper of the host entry on check_cases.arrays' dict under (x, o, e, global)"""
    import wfa_amd
    br = wfa_amd.BatchResult(a["status"], a["score"], a["tbegin"], a["tend"], a["qbegin"], a["qend"], a["align_len"], a["matches"], a["gaps"],
                             a["gap_regions"], a["ops_off"], a["ops_len"], a["ops"])
    kw = dict(penalties=wfa_amd.Penalties(*prm[:3]), options=wfa_amd.Options(GlobalAlignment=bool(prm[3])), mask=mask, n_threads=n_threads)
    return (wfa_amd.check_alignments_packed if packed else wfa_amd.check_alignments)(br, *a["seqs"], **kw)


def _same(got, want, names=None):
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{bad.size} pairs differ; first {i} {names[i] if names else ''}: got {list(got[i])} "
                             f"{sorted(X.names_of(int(got[i][0])))}, want {list(want[i])} {sorted(X.names_of(int(want[i][0])))}")


def test_entries_declared_exported_and_bound(built):
    import wfa_amd
    from wfa_amd import _lib
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    names = ("wfahip_check_alignments_device", "wfahip_check_alignments_packed_device", "wfahip_check_alignments", "wfahip_check_alignments_packed")
    for name in names:
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    dev = ["ctx", "p", "d_rec", "d_ops", "ops_cap", "d_seq_blob", "blob_bytes", "d_q_off", "d_q_len", "d_t_off", "d_t_len", "n_pairs",
           "flag_mask", "d_chk", "d_pass", "n_flagged", "stream"]
    assert args("wfahip_check_alignments_device") == dev
    assert args("wfahip_check_alignments_packed_device") == ["ctx", "p", "d_rec", "d_ops", "ops_cap", "d_packed", "n_words", "d_q_woff", "d_q_len",
                                                             "d_t_woff", "d_t_len", "d_q_rc", "n_pairs", "flag_mask", "d_chk", "d_pass",
                                                             "n_flagged", "stream"]
    assert args("wfahip_check_alignments") == ["r", "p", "seq_blob", "blob_bytes", "q_off", "q_len", "t_off", "t_len", "flag_mask", "n_threads",
                                               "chk", "pass", "n_flagged"]
    assert args("wfahip_check_alignments_packed") == ["r", "p", "packed", "n_words", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "flag_mask",
                                                      "n_threads", "chk", "pass", "n_flagged"]
    assert [len(getattr(_lib.lib(), n).argtypes) for n in names] == [17, 18, 13, 14]
    # the constants: the header's, _lib's and the restatement's
    for k, name in enumerate(X.NAMES):
        assert re.search(r"#define WFAHIP_CHK_%s\s+\(1u << %d\)" % (name, k), hdr), name
        assert getattr(_lib, "CHK_" + name) == getattr(wfa_amd, "CHK_" + name) == X.BIT[name] == 1 << k
    assert _lib.CHK_NAMES == X.NAMES
    assert re.search(r"#define WFAHIP_CHK_ALL\s+\(\(1u << 20\) - 1u\)", hdr) and _lib.CHK_ALL == X.ALL == (1 << 20) - 1
    assert re.search(r"#define WFAHIP_CHK_WORDS 8\b", hdr) and _lib.CHK_WORDS == 8
    assert re.search(r"WFAHIP_PAIR_CHECK_FAILED\s*=\s*16\b", hdr) and _lib.PAIR_CHECK_FAILED == wfa_amd.PAIR_CHECK_FAILED == X.CHECK_FAILED == 16
    assert re.search(r"enum \{ WFAHIP_CHK_W_FLAGS = 0, WFAHIP_CHK_W_COST, WFAHIP_CHK_W_Q_USED, WFAHIP_CHK_W_T_USED, WFAHIP_CHK_W_N_BAD, "
                     r"WFAHIP_CHK_W_FIRST_BAD \};", hdr)
    assert "state what IS, not what is wrong" in raw
    assert _lib.lib().wfahip_version() == 400
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.check_tensors) == ["self", "rec", "ops", "blob", "q_off", "q_len", "t_off", "t_len", "mask", "out", "stream"]
    assert sig(wfa_amd.Aligner.check_tensors_packed) == ["self", "rec", "ops", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "mask",
                                                         "out", "stream"]
    assert sig(wfa_amd.check_alignments)[:6] == ["batch_result", "blob", "q_off", "q_len", "t_off", "t_len"]
    assert sig(wfa_amd.check_alignments_packed)[:7] == ["batch_result", "packed", "q_woff", "q_len", "t_woff", "t_len", "q_rc"]
    for f in (wfa_amd.Aligner.check_tensors, wfa_amd.Aligner.check_tensors_packed, wfa_amd.check_alignments, wfa_amd.check_alignments_packed):
        assert inspect.signature(f).parameters["mask"].default == X.ALL


def test_case_set_is_what_it_claims():
    """every case raises, by the restatement, exactly the flags it is built for; every flag occurs, and occurs with as little
    company as the rule allows; every neighbouring pair of steps meets in some case; the shapes are there"""
    cases = X.cases()
    a = X.arrays(cases)
    chk = X.restate(a, X.PARAMS)
    for c, w in zip(cases, chk):
        assert X.names_of(int(w[0])) == c["claims"], (c["name"], sorted(X.names_of(int(w[0]))))
        if c["status"] != X.OK:
            assert not w.any()
    claims = [c["claims"] for c in cases if c["status"] == X.OK]
    company = {"OPS_RANGE": {"NO_ROWS", "NO_ROWS_TRIMMED"}, "SEQ_RANGE": {"NO_ROWS", "NO_ROWS_TRIMMED"}, "Q_OVER": {"NO_ROWS"},
               "T_OVER": {"NO_ROWS"}}  # what the rule itself adds: a range that fails, or bases that overrun, render no rows
    for name in X.NAMES:
        if name == "NO_ROWS":  # (never without the overrun or the range that causes it)
            assert any(name in s for s in claims)
            continue
        assert frozenset({name} | company.get(name, set())) in claims, name
    assert frozenset() in claims
    together = [("LETTER", "ZERO"), ("ZERO", "UNMERGED"), ("SEQ_RANGE", "Q_OVER"), ("Q_OVER", "M_DIFFERS"), ("T_OVER", "M_DIFFERS"),
                ("M_DIFFERS", "X_EQUAL"), ("M_DIFFERS", "NO_ROWS_TRIMMED"), ("NO_ROWS", "COST_UNDER"), ("COST_UNDER", "STAT_GAP_REGIONS"),
                ("SEQ_RANGE", "COST_OVER"), ("COST_OVER", "STAT_GAPS"), ("X_EQUAL", "COST_OVER")]
    for pair in together:
        assert any(set(pair) <= s for s in claims), pair
    # what a later step must not see: SEQ_RANGE with a differing M column underneath, OPS_RANGE over everything, stale failed pairs
    by = {c["name"]: (c, w) for c, w in zip(cases, chk)}
    c, w = by["range, over, cost"]
    assert c["q"] != by["clean"][0]["q"][:len(c["q"])] and w[4] == 0 and w[5] == X.NONE
    assert list(by["ops range over all"][1]) == [X.BIT["OPS_RANGE"] | X.BIT["NO_ROWS"] | X.BIT["NO_ROWS_TRIMMED"]] + [0] * 7
    assert sorted(c["status"] for c in cases if c["status"] != X.OK) == [1, 2, 4, 8, 101]
    assert all(c["ops_bad"] and c["q_bad"] and c["t_bad"] for c in cases if c["status"] != X.OK)
    assert list(by["m differs"][1][4:6]) == [1, 9] and list(by["x equal"][1][4:6]) == [1, 14]
    assert list(by["m differs and x equal"][1][4:6]) == [4, 5]
    assert list(by["m over, differs inside"][1][1:6]) == [0, 40, 40, 1, 37]
    # saturation: under PARAMS the huge cost leaves 32 bits, under HUGE it leaves 64
    w = by["huge counts"][1]
    assert list(w[1:4]) == [X.M32] * 3
    assert X.cost_of(by["huge counts"][0]["ops"], X.HUGE) > 1 << 64 and X.cost_of([X.op("X", X.M32)], X.HUGE) == (X.M32) ** 2 < 1 << 64
    assert X.restate(a, X.HUGE)[cases.index(by["huge counts"][0])][1] == X.M32
    assert by["huge x"][1][4] == 1 and by["huge x"][1][5] == 9
    assert any(n == 0 for c in cases for _, n in X.split(c["ops"])) and any(n == X.M32 for c in cases for _, n in X.split(c["ops"]))
    # shapes
    assert sorted({len(c["ops"]) for c in cases}) [:1] == [0] and {0, 1, 63, 64, 65, 128, 129, 200} <= {len(c["ops"]) for c in cases}
    assert any(X.sums(c["ops"])[0] >= 70000 and c["status"] == X.OK and len(c["q"]) >= 70000 for c in cases)
    assert {len(c["q"]) % 16 for c in cases if c["name"].startswith("len ")} == set(range(16))
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    ok = np.array([not (c["q_bad"] or c["t_bad"]) for c in cases])
    assert {int(o) % 16 for o in np.concatenate([q_off[ok], t_off[ok]])} == set(range(16))
    assert max(int(o) + int(n) for o, n in zip(np.concatenate([q_off[ok], t_off[ok]]), np.concatenate([q_len[ok], t_len[ok]]))) == len(blob)
    words, q_woff, q_len, t_woff, t_len, q_rc = X.arrays(cases, packed=True, flags=[i & 1 for i in range(len(cases))], junk_tails=9)["seqs"]
    assert max(int(o) + X.packed_words(int(n)) for o, n in zip(np.concatenate([q_woff[ok], t_woff[ok]]),
                                                               np.concatenate([q_len[ok], t_len[ok]]))) == len(words)
    assert q_rc.sum() == len(cases) // 2


@pytest.mark.parametrize("prm", [X.PARAMS, X.PARAMS[:3] + (0,), X.HUGE], ids=["global", "semi-global", "huge-penalties"])
def test_host_entry_on_synthetic_cases(built, prm):
    cases = X.cases()
    names = [c["name"] for c in cases]
    a = X.arrays(cases)
    want = X.restate(a, prm)
    for mask in (X.ALL, X.BIT["NO_ROWS"], 0, X.BIT["M_DIFFERS"] | X.BIT["COST_UNDER"]):
        chk, passed, n_flagged = _host(a, prm, mask=mask)
        _same(chk, want, names)
        want_pass, want_n = X.passed_of(a["status"], want, mask)
        assert np.array_equal(passed, want_pass) and n_flagged == want_n
    if prm[3]:
        assert n_flagged > 3 and (passed == X.CHECK_FAILED).sum() == n_flagged
    else:
        assert not (want[:, 0] & (X.BIT["COST_OVER"] | X.BIT["COST_UNDER"])).any()
    b = X.arrays(cases)  # the inputs were only read
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "seqs") and all(np.array_equal(x, y) for x, y in zip(a["seqs"], b["seqs"]))


@pytest.mark.parametrize("flags", ["none", "all", "alt"])
@pytest.mark.parametrize("junk", [None, 9])
def test_packed_host_entry_on_synthetic_cases(built, flags, junk):
    cases = X.cases()
    n = len(cases)
    fl = {"none": [0] * n, "all": [1] * n, "alt": [i & 1 for i in range(n)]}[flags]
    a = X.arrays(cases, packed=True, flags=fl, junk_tails=junk)
    want = X.restate(a, X.PARAMS, packed=True)
    chk, passed, n_flagged = _host(a, X.PARAMS, packed=True)
    _same(chk, want, [c["name"] for c in cases])
    # the same verdicts as over bytes, but for the packed text entry's rule: no rows are asked of a pair without a column
    bytes_want = X.restate(X.arrays(cases), X.PARAMS)
    differ = np.flatnonzero((want != bytes_want).any(axis=1))
    assert all(X.sums(cases[i]["ops"])[0] == 0 for i in differ)
    want_pass, want_n = X.passed_of(a["status"], want, X.ALL)
    assert np.array_equal(passed, want_pass) and n_flagged == want_n
    if flags == "none":
        chk2, _, _ = _host(dict(a, seqs=a["seqs"][:5] + (None,)), X.PARAMS, packed=True)
        assert np.array_equal(chk2, chk)


def test_threads_give_identical_output(built):
    cases = list(X.cases()) * 3
    a = X.arrays(cases)
    one, eight, many = (_host(a, X.PARAMS, n_threads=t) for t in (1, 8, 1000))
    for x, y in ((one, eight), (one, many)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]


@pytest.mark.parametrize("name", B.CLEAN)
def test_oracles_ordinary_alignments_raise_no_flag(built, name):
    """global 300 bp and 1 kbp @5 % with wf-adaptive 10/50/1 and off, 2/4/2 @10 %, semi-global 200 bp with target overhangs"""
    b = B.batch(name)
    a = X.from_results(b["oracle"], b["seqs"])
    want = X.restate(a, b["prm"])
    chk, passed, n_flagged = _host(a, b["prm"])
    _same(chk, want)
    assert (b["oracle"].status == 0).all() and not chk[:, 0].any() and n_flagged == 0 and not passed.any()
    assert (chk[:, 4] == 0).all() and (chk[:, 5] == X.NONE).all()
    assert np.array_equal(chk[:, 2], b["seqs"][2]) and np.array_equal(chk[:, 3], b["seqs"][4])
    if b["prm"][3]:
        assert np.array_equal(chk[:, 1], b["oracle"].score)
    else:  # semi-global: the ops cover the target's overhangs, the score does not pay for them
        assert (chk[:, 1] > b["oracle"].score).all()
    # ... and from the words, both strands: the flagged queries are packed as their reverse complements
    pk = B.packed(b)
    chk_pk, _, n_pk = _host(dict(a, seqs=pk), b["prm"], packed=True)
    assert np.array_equal(chk_pk, chk) and n_pk == 0 and pk[5].sum() == len(pk[5]) // 2


def test_oracles_alignments_of_short_noisy_pairs_under_aggressive_wf_adaptive(built):
    """40 bases, 20 % errors, wf-adaptive 4/5/1: the reference's own results (the oracle restates them) hold M columns of two
    different bases, ops that overrun a sequence, and CIGARs cheaper than their score.  The flags say so, pair for pair as the
    restatement does."""
    b = B.batch("aggressive")
    a = X.from_results(b["oracle"], b["seqs"])
    want = X.restate(a, b["prm"])
    chk, passed, n_flagged = _host(a, b["prm"])
    _same(chk, want)
    flags = chk[:, 0]
    count = {n: int(((flags & X.BIT[n]) != 0).sum()) for n in X.NAMES}
    print("aggressive batch:", {k: v for k, v in count.items() if v}, "of", len(flags))
    assert count["M_DIFFERS"] >= 1 and count["Q_OVER"] + count["T_OVER"] >= 1 and count["COST_UNDER"] >= 1
    assert n_flagged == int((flags != 0).sum()) and 0 < n_flagged < len(flags) // 20
    for n in ("OPS_RANGE", "LETTER", "ZERO", "UNMERGED", "SEQ_RANGE", "X_EQUAL", "COST_OVER", "STAT_ALIGN_LEN", "STAT_MATCHES", "STAT_GAPS",
              "STAT_GAP_REGIONS"):
        assert count[n] == 0, n
    over = (flags & (X.BIT["Q_OVER"] | X.BIT["T_OVER"])) != 0
    assert ((flags[over] & X.BIT["NO_ROWS"]) != 0).all()
    pk = B.packed(b)
    chk_pk, _, _ = _host(dict(a, seqs=pk), b["prm"], packed=True)
    assert np.array_equal(chk_pk, chk)


def _results(a):
    from wfa_amd import _lib
    r = _lib.Results()
    r.n, r.n_ops = len(a["status"]), len(a["ops"])
    for k, t in (("status", C.c_int32), ("tbegin", C.c_int32), ("tend", C.c_int32), ("qbegin", C.c_int32), ("qend", C.c_int32),
                 ("score", C.c_uint32), ("align_len", C.c_uint32), ("matches", C.c_uint32), ("gaps", C.c_uint32), ("gap_regions", C.c_uint32),
                 ("ops_len", C.c_uint32), ("ops_off", C.c_uint64), ("ops", C.c_uint64)):
        setattr(r, k, a[k].ctypes.data_as(C.POINTER(t)))
    return r


def test_host_entry_checks(built):
    from wfa_amd import _lib
    f, BAD = _lib.lib().wfahip_check_alignments, _lib.ERR_BAD_ARG
    cases = list(X.cases()[:3])
    a = X.arrays(cases)
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    prm = _lib.Params(4, 6, 2, 1, 0)
    chk, passed, cnt = np.full((3, 8), 7, np.uint32), np.full(3, 7, np.int32), C.c_uint64(99)

    def call(r=None, null=(), p=prm, **kw):
        r = r if r is not None else _results(a)
        args = dict(r=C.byref(r), p=C.byref(p) if p is not None else None, blob=vp(blob), blob_bytes=len(blob), q_off=vp(q_off), q_len=vp(q_len),
                    t_off=vp(t_off), t_len=vp(t_len), mask=X.ALL, n_threads=2, chk=vp(chk), passed=vp(passed), cnt=C.byref(cnt))
        args.update(kw)
        for k in null:
            args[k] = None
        return f(*args.values())
    assert call() == 0 and cnt.value == 2 and np.array_equal(chk, X.restate(a, X.PARAMS))
    assert call(null=("passed", "cnt")) == 0
    for k in ("r", "p", "chk", "q_off", "q_len", "t_off", "t_len", "blob"):
        assert call(null=(k,)) == BAD, k
    for k in ("status", "score", "tbegin", "tend", "qbegin", "qend", "align_len", "matches", "gaps", "gap_regions", "ops_off", "ops_len", "ops"):
        r = _results(a)
        setattr(r, k, None)
        assert call(r=r) == BAD, k
    assert call(p=_lib.Params(0, 6, 2, 1, 0)) == _lib.ERR_UNSUPPORTED and call(p=_lib.Params(4, 0, 0, 1, 0)) == _lib.ERR_UNSUPPORTED
    assert call(p=_lib.Params(4, 6, 2, 1, 1, (C.c_uint8 * 2)(), 0, 50, 1)) == BAD  # wf-adaptive with min_wf_len 0
    r = _results(a)
    r.n = 0xFFFFFFF1
    assert call(r=r) == BAD
    # an empty result: OK, the count 0, nothing touched; null arrays are fine then
    chk[:], cnt.value = 7, 99
    r = _lib.Results()
    assert call(r=r, null=("q_off", "q_len", "t_off", "t_len", "blob"), blob_bytes=0) == 0 and cnt.value == 0 and (chk == 7).all()
    assert call(r=r, null=("chk",)) == BAD
    # n_threads below 1 is one thread
    chk[:] = 7
    assert call(n_threads=0) == 0 and np.array_equal(chk, X.restate(a, X.PARAMS))
    # the packed entry likewise
    g = _lib.lib().wfahip_check_alignments_packed
    pa = X.arrays(cases, packed=True, flags=[0, 1, 0])
    words, q_woff, q_len2, t_woff, t_len2, q_rc = pa["seqs"]
    ok = [C.byref(_results(pa)), C.byref(prm), vp(words), len(words), vp(q_woff), vp(q_len2), vp(t_woff), vp(t_len2), vp(q_rc), X.ALL, 2, vp(chk),
          vp(passed), C.byref(cnt)]
    assert g(*ok) == 0 and np.array_equal(chk, X.restate(pa, X.PARAMS, packed=True))
    for k in (0, 1, 2, 4, 5, 6, 7, 11):
        assert g(*[None if j == k else v for j, v in enumerate(ok)]) == BAD, k
    assert g(*[None if j in (8, 12, 13) else v for j, v in enumerate(ok)]) == 0  # flags, pass and count may be null
    # fewer words than the sequences need: a flag, not an error
    short = list(ok)
    short[3] = len(words) - 1
    assert g(*short) == 0 and np.array_equal(chk, X.restate(pa, X.PARAMS, packed=True, n_words=len(words) - 1))
    assert (chk[:, 0] & X.BIT["SEQ_RANGE"]).any()


def test_device_entries_bad_args_without_device(built):
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG
    ctx, p = C.c_void_p(1), C.c_void_p(4096)  # (everything below returns before the context -- the address 1 -- or a buffer is dereferenced)
    prm = _lib.Params(4, 6, 2, 1, 0)
    cnt = C.c_uint64(99)
    for f, extra in ((_lib.lib().wfahip_check_alignments_device, []), (_lib.lib().wfahip_check_alignments_packed_device, [p])):
        ok = [ctx, C.byref(prm), p, p, 8, p, 8, p, p, p, p] + extra + [1, X.ALL, p, p, C.byref(cnt), None]
        n_at = 11 + len(extra)

        def call(**kw):
            a = list(ok)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return f(*a)
        for k in (0, 1, n_at + 2):                           # ctx, p, d_chk
            assert call(**{f"a{k}": None}) == BAD, k
            assert call(**{f"a{k}": None, f"a{n_at}": 0}) == BAD, k   # ... whatever n_pairs is
        for k in (2, 7, 8, 9, 10):                           # d_rec, the offset and length arrays
            assert call(**{f"a{k}": None}) == BAD, k
        assert call(a3=None) == BAD                          # d_ops null with ops_cap > 0
        assert call(a5=None) == BAD                          # the blob / the words null with a size
        assert call(**{f"a{n_at}": 0xFFFFFFF1}) == BAD
        assert cnt.value == 99
        bad_prm = _lib.Params(0, 6, 2, 1, 0)
        assert call(a1=C.byref(bad_prm)) == _lib.ERR_UNSUPPORTED and cnt.value == 99
        # an empty batch touches nothing: not the context, not the device
        assert call(a2=None, a3=None, a4=0, a5=None, a6=0, a7=None, a8=None, a9=None, a10=None, **{f"a{n_at}": 0}) == 0 and cnt.value == 0
        cnt.value = 99
        assert call(**{f"a{n_at}": 0, f"a{n_at + 4}": None}) == 0 and cnt.value == 99


def test_python_wrappers_refuse_wrong_shapes_before_the_call(built):
    import torch
    import wfa_amd
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    cpu = lambda shape, dt: torch.zeros(shape, dtype=dt)
    good = (cpu((2, 16), torch.int32), cpu(4, torch.int64), cpu(8, torch.uint8), cpu(2, torch.int64), cpu(2, torch.int32),
            cpu(2, torch.int64), cpu(2, torch.int32))
    with pytest.raises(ValueError):
        al.check_tensors(*good)                                                     # on the host
    with pytest.raises(ValueError):
        al.check_tensors_packed(np.zeros((2, 16), np.int32), *good[1:])             # numpy arrays
    a = X.arrays(list(X.cases()[:2]))
    br = wfa_amd.BatchResult(a["status"], a["score"], a["tbegin"], a["tend"], a["qbegin"], a["qend"], a["align_len"], a["matches"], a["gaps"],
                             a["gap_regions"], a["ops_off"], a["ops_len"], a["ops"])
    seqs = a["seqs"]
    chk, passed, n = wfa_amd.check_alignments(br, *seqs, penalties=wfa_amd.Penalties(4, 6, 2))
    assert chk.shape == (2, 8) and chk.dtype == np.uint32 and passed.dtype == np.int32 and n == 1
    with pytest.raises(ValueError):
        wfa_amd.check_alignments(br, *seqs, n_threads=0)
    with pytest.raises(ValueError):
        wfa_amd.check_alignments(br, *seqs, mask=1 << 32)
    with pytest.raises(ValueError):
        wfa_amd.check_alignments(br, seqs[0], seqs[1][:1], *seqs[2:])
    with pytest.raises(ValueError):
        wfa_amd.check_alignments(br, seqs[0].reshape(1, -1), *seqs[1:])
    br.matches = np.zeros(3, np.uint32)
    with pytest.raises(ValueError):
        wfa_amd.check_alignments(br, *seqs)


def test_rule_under_sanitizers():
    src = os.path.join(ROOT, "tests", "check_host_test.cpp")
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    for name, flags in (("check_host_test", []), ("check_host_test_asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(ROOT, "build", name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "check host test ok" in r.stdout
