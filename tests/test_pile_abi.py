"""CPU: the pileup (include/wfa_hip.h: wfahip_pileup_device, wfahip_pileup_packed_device, wfahip_pileup, wfahip_pileup_packed).  The
entries' declarations, bindings and constants; the host entries -- the same header functions as the kernels -- against the numpy
restatement of tests/pile_cases.py on the synthetic set of tests/check_cases.py, on the oracle's alignments of tests/check_batches.py
and on a batch of 8 targets that 40 reads each share, from bytes and from words on both strands; what the counters must add up to;
windows, tiles and accumulation; every argument error, before a context or a device is touched."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import check_batches as B  # noqa: E402
import check_cases as X  # noqa: E402
import pile_cases as P  # noqa: E402

CANARY = 0xC0FFEE01


def _results(a, null=()):
    from wfa_amd import _lib
    r = _lib.Results()
    r.n, r.n_ops = len(a["status"]), len(a["ops"])
    keep = []
    for f, ct, dt in (("status", C.c_int32, np.int32), ("ops_off", C.c_uint64, np.uint64), ("ops_len", C.c_uint32, np.uint32),
                      ("ops", C.c_uint64, np.uint64), ("qbegin", C.c_int32, np.int32), ("qend", C.c_int32, np.int32),
                      ("tbegin", C.c_int32, np.int32), ("tend", C.c_int32, np.int32)):
        arr = np.ascontiguousarray(a[f], dtype=dt)
        keep.append(arr)
        setattr(r, f, None if f in null else arr.ctypes.data_as(C.POINTER(ct)))
    return r, keep


def _call(a, only, pile_at, pile_n, packed=False, n_threads=3, null=(), size=None, counts=None, flags=True):
    """the C host entry on a check_cases dict: (return code, counts uint32 [pile_n + 2, 8] with a canary row before and behind the
    window's, n_piled)"""
    from wfa_amd import _lib
    r, keep = _results(a, null)
    vp = lambda name, x: None if name in null else np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    if counts is None:
        counts = np.zeros((pile_n + 2, 8), np.uint32)
        counts[0] = counts[-1] = CANARY
    cnt = C.c_uint64(777)
    seqs, q_off, q_len, t_off, t_len = a["seqs"][:5]
    told = len(seqs) if size is None else size
    held = np.ascontiguousarray(seqs[:told]) if told <= len(seqs) else np.ascontiguousarray(seqs)
    tail = (only, n_threads, pile_at, pile_n, None if "counts" in null else counts[1:].ctypes.data_as(C.c_void_p), C.byref(cnt))
    args = [C.byref(r), vp("seqs", held), told, vp("q_off", q_off), vp("q_len", q_len), vp("t_off", t_off), vp("t_len", t_len)]
    if packed:
        q_rc = a["seqs"][5] if flags and len(a["seqs"]) > 5 else None
        rc = _lib.lib().wfahip_pileup_packed(*args, None if q_rc is None else vp("q_rc", q_rc), *tail)
    else:
        rc = _lib.lib().wfahip_pileup(*args, *tail)
    return rc, counts, cnt.value


def _same(counts, want, what=""):
    assert (counts[0] == CANARY).all() and (counts[-1] == CANARY).all(), "a counter outside the window was written"
    bad = np.argwhere(counts[1:-1] != want)
    assert bad.size == 0, f"{what}: first differing counter (base, word) {bad[0]}: got {counts[1:-1][tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def test_entries_declared_exported_and_bound(built):
    import wfa_amd
    from wfa_amd import _lib
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    names = ("wfahip_pileup_device", "wfahip_pileup_packed_device", "wfahip_pileup", "wfahip_pileup_packed")
    for name in names:
        assert name in declared and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    args = lambda name: [a.strip().split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert args("wfahip_pileup_device") == ["ctx", "d_rec", "d_ops", "ops_cap", "d_seq_blob", "blob_bytes", "d_q_off", "d_q_len", "d_t_off",
                                            "d_t_len", "n_pairs", "only_aligned", "pile_at", "pile_n", "d_counts", "n_piled", "stream"]
    assert args("wfahip_pileup_packed_device") == ["ctx", "d_rec", "d_ops", "ops_cap", "d_packed", "n_words", "d_q_woff", "d_q_len", "d_t_woff",
                                                   "d_t_len", "d_q_rc", "n_pairs", "only_aligned", "pile_at", "pile_n", "d_counts", "n_piled",
                                                   "stream"]
    assert args("wfahip_pileup") == ["r", "seq_blob", "blob_bytes", "q_off", "q_len", "t_off", "t_len", "only_aligned", "n_threads", "pile_at",
                                     "pile_n", "counts", "n_piled"]
    assert args("wfahip_pileup_packed") == ["r", "packed", "n_words", "q_woff", "q_len", "t_woff", "t_len", "q_rc", "only_aligned", "n_threads",
                                            "pile_at", "pile_n", "counts", "n_piled"]
    L = _lib.lib()
    assert [len(getattr(L, f).argtypes) for f in names] == [17, 18, 13, 14]
    assert L.wfahip_version() == 400 and "#define WFAHIP_VERSION 400" in raw
    # the constants: the header's, the package's and the restatement's
    assert re.search(r"#define\s+WFAHIP_PILE_WORDS\s+8\b", raw)
    enum = re.search(r"enum\s*\{\s*(WFAHIP_PILE_W_A\s*=\s*0[^}]*)\}", hdr).group(1)
    order = [re.sub(r"\s*=\s*0", "", x.strip()) for x in enum.split(",")]
    assert order == ["WFAHIP_PILE_W_" + n for n in P.NAMES]
    assert _lib.PILE_WORDS == wfa_amd.PILE_WORDS == P.WORDS == 8 and _lib.PILE_NAMES == wfa_amd.PILE_NAMES == P.NAMES
    for k, n in enumerate(P.NAMES):
        assert getattr(_lib, "PILE_W_" + n) == getattr(wfa_amd, "PILE_W_" + n) == getattr(P, n) == k
    assert [(b >> 1) & 3 for b in b"ACTG"] == [0, 1, 2, 3] == [(b >> 1) & 3 for b in b"actg"]
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(wfa_amd.Aligner.pileup_tensors) == ["self", "rec", "ops", "blob", "q_off", "q_len", "t_off", "t_len", "pile_at", "pile_n",
                                                   "only_aligned", "out", "stream"]
    assert sig(wfa_amd.Aligner.pileup_tensors_packed) == ["self", "rec", "ops", "packed", "q_woff", "q_len", "t_woff", "t_len", "pile_at",
                                                          "pile_n", "q_rc", "only_aligned", "out", "stream"]
    assert sig(wfa_amd.pileup) == ["batch_result", "blob", "q_off", "q_len", "t_off", "t_len", "pile_at", "pile_n", "only_aligned", "n_threads",
                                   "out"]
    assert sig(wfa_amd.pileup_packed) == ["batch_result", "packed", "q_woff", "q_len", "t_woff", "t_len", "pile_at", "pile_n", "q_rc",
                                          "only_aligned", "n_threads", "out"]
    for f in (wfa_amd.Aligner.pileup_tensors, wfa_amd.Aligner.pileup_tensors_packed, wfa_amd.pileup, wfa_amd.pileup_packed):
        p = inspect.signature(f).parameters
        assert p["only_aligned"].default is False and p["out"].default is None
    assert inspect.signature(wfa_amd.pileup_packed).parameters["q_rc"].default is None


def test_restatement_by_hand():
    """the rule on one pair small enough to count by hand: query GATTACA over target bytes 10 .. 18 of a blob, ops 2D 3M 1X 2I 1M 1H
    then 1D.  The leading D run sits in front of the window's first base and shares base 0's counters"""
    op = X.op
    ops = [op("D", 2), op("M", 3), op("X", 1), op("I", 2), op("M", 1), op("D", 1), op("H", 1)]
    blob = np.frombuffer(b"GATTACAnnn" + b"TTAGGGCxx" + b"z", np.uint8)  # query at 0 (7 + an n it does not use), target at 10
    a = dict(status=np.zeros(1, np.int32), ops_off=np.zeros(1, np.uint64), ops_len=np.array([len(ops)], np.uint32), ops=np.array(ops, np.uint64),
             qbegin=np.array([3], np.int32), qend=np.array([7], np.int32), tbegin=np.array([1], np.int32), tend=np.array([7], np.int32),
             seqs=(blob, np.zeros(1, np.uint64), np.array([9], np.uint32), np.array([10], np.uint64), np.array([7], np.uint32)))
    counts, n_piled = P.restate(a, 8, 12, 0)
    want = np.zeros((12, 8), np.uint32)
    # query GA|TTA|C|A|n then H: D GA -> base 10 (ts = 0 -> base 0 of the target window); M TTA over 10 11 12; X C over 13;
    # I over 14 15; M A over 16; D n behind base 16; H nothing
    want[10 - 8, [P.EXTRA, P.EXTRA_BASES]] = [1, 2]
    want[10 - 8, P.T] += 1
    want[11 - 8, P.T] += 1
    want[12 - 8, P.A] += 1
    want[13 - 8, P.C] += 1
    want[14 - 8, P.GAP] += 1
    want[15 - 8, P.GAP] += 1
    want[16 - 8, P.A] += 1
    want[16 - 8, [P.EXTRA, P.EXTRA_BASES]] = [1, 1]
    assert n_piled == 1 and np.array_equal(counts, want)
    # trimmed: the first M op to the last over the record's windows -- query bases [2, 7), target bases [0, 7)
    counts, n_piled = P.restate(a, 8, 12, 1)
    want[10 - 8, [P.EXTRA, P.EXTRA_BASES]] = 0
    want[16 - 8, [P.EXTRA, P.EXTRA_BASES]] = 0
    assert n_piled == 1 and np.array_equal(counts, want)
    # 'n' is OTHER
    a["ops"] = np.array([op("M", 7), op("X", 1)], np.uint64)
    a["ops_len"][0] = 2
    a["seqs"] = (blob, np.zeros(1, np.uint64), np.array([8], np.uint32), np.array([10], np.uint64), np.array([8], np.uint32))
    counts, _ = P.restate(a, 17, 1, 0)
    assert counts.tolist() == [[0, 0, 0, 0, 1, 0, 0, 0]]


@pytest.mark.parametrize("n_threads", [1, 8])
@pytest.mark.parametrize("only", [0, 1])
def test_host_entries_on_the_synthetic_set_bytes(built, only, n_threads):
    """check_cases.cases(): op lists of 0, 1, 63, 64, 65, 128, 129 and 200 ops, an op of 70 001 columns, unknown letters, counts of
    0.  The set holds pairs that fail a check: as it is the call is refused, counts untouched; with them set aside -- and the
    offsets of every pair that is not OK poisoned -- it equals the restatement"""
    from wfa_amd import _lib
    cs = X.cases()
    assert {len(c["ops"]) for c in cs} >= set(X.N_OPS)
    a = X.arrays(cs)
    at, n = P.span(a)
    assert P.restate(a, at, n, only) is None
    rc, counts, piled = _call(a, only, at, n, n_threads=n_threads)
    assert rc == _lib.ERR_BAD_ARG and not counts[1:-1].any() and piled == 0
    b, aside = P.set_aside(a, only)
    assert aside and len(aside) < len(cs) // 2
    want, want_piled = P.restate(b, at, n, only)
    assert want.any() and want_piled > len(cs) // 2
    rc, counts, piled = _call(b, only, at, n, n_threads=n_threads)
    assert rc == 0 and piled == want_piled
    _same(counts, want)
    c = X.arrays(cs)  # the inputs were only read
    assert all(np.array_equal(a[k], c[k]) for k in ("status", "ops_off", "ops_len", "ops"))
    assert all(np.array_equal(x, y) for x, y in zip(a["seqs"], c["seqs"]))


@pytest.mark.parametrize("flags", ["none", "alt"])
@pytest.mark.parametrize("only", [0, 1])
def test_host_entries_on_the_synthetic_set_words(built, flags, only):
    from wfa_amd import _lib
    cs = X.cases()
    a = X.arrays(cs, packed=True, flags=[(i & 1) if flags == "alt" else 0 for i in range(len(cs))], junk_tails=9)
    at, n = P.span(a, packed=True)
    assert P.restate(a, at, n, only, packed=True) is None
    rc, counts, piled = _call(a, only, at, n, packed=True)
    assert rc == _lib.ERR_BAD_ARG and not counts[1:-1].any()
    b, aside = P.set_aside(a, only, packed=True)
    want, want_piled = P.restate(b, at, n, only, packed=True)
    rc, counts, piled = _call(b, only, at, n, packed=True, n_threads=5)
    assert rc == 0 and piled == want_piled and not want[:, P.OTHER].any()
    _same(counts, want)
    if flags == "none":  # a null flag array is the array of zeros
        rc, counts, piled = _call(b, only, at, n, packed=True, flags=False)
        assert rc == 0 and piled == want_piled
        _same(counts, want)


def _real(name):
    b = B.batch(name)
    return b, X.from_results(b["oracle"], b["seqs"]), X.from_results(b["oracle"], B.packed(b))


def _invariants(a, counts, only, packed):
    """what a window over everything must add up to"""
    tot = {k: 0 for k in "MXID"}
    n_d = 0
    for i in range(len(a["status"])):
        p = P.pair_plan(a, i, only, packed)
        if not p or not p[4]:
            continue
        ops, _, T0, t_n, _ = p
        for letter, n in ops:
            if chr(letter) in tot:
                tot[chr(letter)] += n
            n_d += 1 if letter == ord("D") and n else 0
        if i % 9 == 0:  # per pair, words 0 .. 5 over its target equal T_USED -- on a pileup of that pair alone
            one = P.restate(_only_pair(a, i), T0, t_n, only, packed)[0]
            assert int(one[:, :6].sum()) == sum(n for l, n in ops if l in b"MXI")
    c = counts.astype(np.uint64)
    assert int(c[:, :5].sum()) == tot["M"] + tot["X"]
    assert int(c[:, P.GAP].sum()) == tot["I"]
    assert int(c[:, P.EXTRA].sum()) == n_d
    assert int(c[:, P.EXTRA_BASES].sum()) == tot["D"]


def _only_pair(a, i):
    b = {k: (v[i:i + 1] if k not in ("ops", "seqs") else v) for k, v in a.items() if k != "rec"}
    b["seqs"] = (a["seqs"][0],) + tuple(x[i:i + 1] for x in a["seqs"][1:])
    return b


@pytest.mark.parametrize("name", B.CLEAN)
def test_host_entries_on_the_oracles_alignments(built, name):
    """trimmed (the wf-adaptive pair that overruns its sequences is refused untrimmed: tests/test_diff_abi.py) and, with the pairs the
    restatement finds failing set aside, untrimmed; from bytes and from words, position for position"""
    b, by, pk = _real(name)
    for only in (1, 0):
        by2, aside = P.set_aside(by, only)
        pk2, aside_pk = P.set_aside(pk, only, packed=True)
        assert aside == aside_pk and len(aside) <= 2
        at, n = P.span(by2)
        want, want_piled = P.restate(by2, at, n, only)
        rc, counts, piled = _call(by2, only, at, n, n_threads=8)
        assert rc == 0 and piled == want_piled >= len(by["status"]) - 2
        _same(counts, want, name)
        # the packed result equals the byte result position for position: base p of the sequence at word w is 16 w + p
        at_pk, n_pk = P.span(pk2, packed=True)
        want_pk, _ = P.restate(pk2, at_pk, n_pk, only, packed=True)
        rc, counts_pk, piled_pk = _call(pk2, only, at_pk, n_pk, packed=True, n_threads=8)
        assert rc == 0 and piled_pk == want_piled
        _same(counts_pk, want_pk, name + " packed")
        for i in range(0, len(by["status"]), 7):
            to, tw, tl = int(by["seqs"][3][i]), int(pk["seqs"][3][i]), int(by["seqs"][4][i])
            assert np.array_equal(counts[1:-1][to:to + tl], counts_pk[1:-1][16 * tw:16 * tw + tl]), i
    if name in ("global 300", "semi-global 200"):
        _invariants(by2, counts[1:-1], 0, False)


def test_shared_targets(built):
    """8 targets, 40 reads each, t_off repeated: depth, windows, tiles, accumulation; bytes and words with every second query flagged"""
    S = P.shared_targets()
    by, pk = S["bytes"], S["words"]
    assert (by["status"] == 0).all()
    at, n = P.span(by)
    for only in (0, 1):
        want, want_piled = P.restate(by, at, n, only)
        rc, counts, piled = _call(by, only, at, n, n_threads=8)
        assert rc == 0 and piled == want_piled == len(by["status"])
        _same(counts, want)
        at_pk, n_pk = P.span(pk, packed=True)
        want_pk, _ = P.restate(pk, at_pk, n_pk, only, packed=True)
        rc, counts_pk, piled = _call(pk, only, at_pk, n_pk, packed=True, n_threads=8)
        assert rc == 0 and piled == want_piled
        _same(counts_pk, want_pk)
        for to, tw, tl in S["targets"]:
            cov = counts[1:-1][to:to + tl]
            assert np.array_equal(cov, counts_pk[1:-1][16 * tw:16 * tw + tl])
            if only == 0:  # a global alignment covers every base of its target once: words 0 .. 5 sum to the depth
                assert (cov[:, :6].sum(axis=1) == S["depth"]).all()
        _invariants(by, counts[1:-1], only, False)
    # a window that starts and ends inside a target (and inside ops), two tiles, and a second call that doubles
    to, _, tl = S["targets"][3]
    whole, _ = P.restate(by, at, n, 0)
    rc, part, _ = _call(by, 0, to + 17, 101)
    assert rc == 0
    _same(part, whole[to + 17:to + 118])
    rc, left, _ = _call(by, 0, at, to + 50)
    rc2, right, _ = _call(by, 0, to + 50, n - (to + 50))
    assert rc == rc2 == 0 and np.array_equal(np.concatenate([left[1:-1], right[1:-1]]), whole)
    rc, twice, _ = _call(by, 0, to + 17, 101, counts=part)
    assert rc == 0
    _same(twice, 2 * whole[to + 17:to + 118])
    # a window outside the blob receives nothing; every pair is still swept
    rc, none, piled = _call(by, 0, len(by["seqs"][0]) + 5, 64)
    assert rc == 0 and not none[1:-1].any() and piled == len(by["status"])
    rc, none, piled = _call(by, 0, (1 << 64) - 64, 64)
    assert rc == 0 and not none[1:-1].any()


def test_python_wrappers(built):
    import wfa_amd
    S = P.shared_targets()
    by, pk, w = S["bytes"], S["words"], S["oracle"]
    br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions, w.ops_off,
                             w.ops_len, w.ops)
    to, tw, tl = S["targets"][2]
    want, _ = P.restate(by, to, tl, 1)
    got = wfa_amd.pileup(br, *by["seqs"], to, tl, only_aligned=True, n_threads=3)
    assert got.dtype == np.uint32 and got.shape == (tl, 8) and np.array_equal(got, want)
    got_pk = wfa_amd.pileup_packed(br, *pk["seqs"][:5], 16 * tw, tl, q_rc=pk["seqs"][5], only_aligned=True)
    assert np.array_equal(got_pk, want)
    again = wfa_amd.pileup(br, *by["seqs"], to, tl, only_aligned=True, out=got)
    assert again is got and np.array_equal(got, 2 * want)
    assert wfa_amd.pileup(br, *by["seqs"], 0, 0).shape == (0, 8)
    with pytest.raises(ValueError):
        wfa_amd.pileup(br, *by["seqs"], to, tl, n_threads=0)
    with pytest.raises(ValueError):
        wfa_amd.pileup(br, *by["seqs"], to, tl, out=np.zeros((tl, 8), np.int32))
    with pytest.raises(ValueError):
        wfa_amd.pileup(br, *by["seqs"], to, tl, out=np.zeros((tl + 1, 8), np.uint32))
    with pytest.raises(ValueError):
        wfa_amd.pileup(br, *by["seqs"], -1, tl)
    with pytest.raises(ValueError):
        wfa_amd.pileup(br, *by["seqs"], 0, (1 << 58) + 1)
    with pytest.raises(ValueError):
        wfa_amd.pileup(br, by["seqs"][0], by["seqs"][1][:2], *by["seqs"][2:], to, tl)
    with pytest.raises(ValueError):
        wfa_amd.pileup_packed(br, *pk["seqs"][:5], 0, 16, q_rc=pk["seqs"][5][:3])
    import torch
    al = object.__new__(wfa_amd.Aligner)  # (no context: refused before the C entry is reached)
    cpu = lambda shape, dt: torch.zeros(shape, dtype=dt)
    with pytest.raises(ValueError):
        al.pileup_tensors(cpu((2, 16), torch.int32), cpu(4, torch.int64), cpu(8, torch.uint8), cpu(2, torch.int64), cpu(2, torch.int32),
                          cpu(2, torch.int64), cpu(2, torch.int32), 0, 8)   # on the host
    with pytest.raises(ValueError):
        al.pileup_tensors_packed(cpu((2, 16), torch.int32), cpu(4, torch.int64), cpu(8, torch.int32), cpu(2, torch.int64), cpu(2, torch.int32),
                                 cpu(2, torch.int64), cpu(2, torch.int32), 0, 8)


def _one(packed=False, **kw):
    """one clean pair of check_cases (BASE_OPS) as arrays, a field of the record or an offset / length replaced"""
    c = X.cases()[0]
    a = X.arrays([c], packed=packed, flags=[1] if packed else None)
    for k, v in kw.items():
        if k in ("q_off", "q_len", "t_off", "t_len"):
            seqs = [np.array(x) for x in a["seqs"]]
            seqs[1 + ("q_off", "q_len", "t_off", "t_len").index(k)][0] = v
            a["seqs"] = tuple(seqs)
        else:
            a[k] = a[k].copy()
            a[k][0] = v
    return a


@pytest.mark.parametrize("packed", [False, True])
def test_host_entry_checks(built, packed):
    """every check next to the same input at its bound: WFAHIP_ERR_BAD_ARG with counts untouched, and a pass"""
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG
    base = _one(packed)
    at, n = P.span(base, packed)

    def bad(only, a, **kw):
        assert P.restate(a, at, n, only, packed, size=kw.get("size")) is None or kw.get("null") or kw.get("n_big")
        counts = np.zeros((n + 2, 8), np.uint32)
        counts[0] = counts[-1] = CANARY
        rc, counts, piled = _call(a, only, at, kw.pop("n_big", n), packed=packed, counts=counts, **kw)
        assert rc == BAD and not counts[1:-1].any() and (counts[0] == CANARY).all() and (counts[-1] == CANARY).all()

    def good(only, a, **kw):
        want, want_piled = P.restate(a, at, n, only, packed, size=kw.get("size"))
        rc, counts, piled = _call(a, only, at, n, packed=packed, **kw)
        assert rc == 0 and piled == want_piled == 1
        _same(counts, want)
    r = X.cases()[0]["rec"]
    seqs, q_off, q_len, t_off, t_len = base["seqs"][:5]
    ql, tl = int(q_len[0]), int(t_len[0])
    for only in (0, 1):
        good(only, base)
        # the blob (the words): the later sequence ends on its last byte (pad word)
        good(only, base, size=len(seqs))
        bad(only, base, size=len(seqs) - 1)
        bad(only, base, size=0)
        last = "q_off" if q_off[0] > t_off[0] else "t_off"
        for v in (int(base["seqs"][1 if last == "q_off" else 3][0]) + 1, len(seqs), 1 << 63, (1 << 64) - 1):
            bad(only, _one(packed, **{last: v}))
        # the op range one past the op buffer
        n_ops = len(base["ops"])
        bad(only, _one(packed, ops_off=n_ops - int(base["ops_len"][0]) + 1))
        bad(only, _one(packed, ops_len=n_ops + 1, ops_off=0))
        bad(only, _one(packed, ops_off=1 << 63))
    # the ops consume one base more than the sequence holds (BASE_OPS ends ... 1X 2D: untrimmed both overrun, trimmed neither)
    bad(0, _one(packed, q_len=ql - 1))
    bad(0, _one(packed, t_len=tl - 1))
    good(1, _one(packed, q_len=ql - 1))
    good(1, _one(packed, t_len=tl - 1))
    # the trimmed windows
    bad(1, _one(packed, qend=r["qend"] - 1))
    bad(1, _one(packed, tbegin=r["tbegin"] + 1))
    good(1, _one(packed, qbegin=r["qbegin"] - 1))
    bad(1, _one(packed, qbegin=0, qend=r["qend"] - r["qbegin"]))
    bad(1, _one(packed, tbegin=0, tend=r["tend"] - r["tbegin"]))
    bad(1, _one(packed, qbegin=-3))
    bad(1, _one(packed, qend=ql + 1))
    bad(1, _one(packed, tend=tl + 1))
    bad(1, _one(packed, qbegin=r["qend"] + 2))
    good(0, _one(packed, qbegin=0, qend=-1, tbegin=77, tend=-5))
    # null arguments
    for name in ("status", "ops_off", "ops_len", "ops", "seqs", "q_off", "q_len", "t_off", "t_len", "counts"):
        bad(0, base, null=(name,))
    for name in ("qbegin", "qend", "tbegin", "tend"):
        bad(1, base, null=(name,))
        good(0, base, null=(name,))
    bad(0, base, n_big=(1 << 58) + 1)
    f = _lib.lib().wfahip_pileup_packed if packed else _lib.lib().wfahip_pileup
    nulls = [None, 0, None, None, None, None] + ([None] if packed else [])
    cnt = C.c_uint64(5)
    word = np.full(8, CANARY, np.uint32)
    assert f(None, *nulls, 0, 1, 0, 1, word.ctypes.data_as(C.c_void_p), C.byref(cnt)) == BAD and cnt.value == 5
    # no pairs, or no window: nothing is touched, whatever else is null
    assert f(C.byref(_lib.Results()), *nulls, 1, 4, 0, 1, word.ctypes.data_as(C.c_void_p), C.byref(cnt)) == 0 and cnt.value == 0
    assert (word == CANARY).all()
    cnt.value = 5
    rc, counts, piled = _call(base, 0, at, 0, packed=packed, null=("counts",))
    assert rc == 0 and piled == 0
    rc, counts, piled = _call(base, 0, at, n, packed=packed)
    assert rc == 0 and piled == 1
    assert f(C.byref(_lib.Results()), *nulls, 1, 4, 0, 0, None, None) == 0


def test_offsets_of_pairs_that_add_nothing_are_never_looked_at(built):
    """not OK, no op, trimmed no M op -- and, packed, no column: offsets far outside the buffer, nothing refused"""
    rng = np.random.default_rng(3)
    no_m = X.clean("no M", [X.op("X", 2), X.op("I", 1), X.op("D", 1)], rng)
    cs = [X.cases()[0], X.changed(X.cases()[0], "not ok", [], status=4), X.clean("empty", [], rng), no_m,
          X.clean("no column", [X.op("~", 9), X.op("Z", 1)], rng)]
    for packed in (False, True):
        a = X.arrays(cs, packed=packed, flags=[0, 1, 0, 1, 0] if packed else None)
        seqs = [np.array(x) for x in a["seqs"]]
        for i in (1, 2) + ((4,) if packed else ()):
            seqs[1][i] = seqs[3][i] = P.POISON
            seqs[2][i] = seqs[4][i] = 1000
        a["seqs"] = tuple(seqs)
        at, n = P.span(a, packed)
        for only in (0, 1):
            if only:
                seqs[1][3] = seqs[3][3] = P.POISON
            want, want_piled = P.restate(a, at, n, only, packed)
            rc, counts, piled = _call(a, only, at, n, packed=packed)
            assert rc == 0 and piled == want_piled == (1 if only else 2)
            _same(counts, want)


def test_the_wf_adaptive_pair_that_overruns_is_refused_untrimmed_and_set_aside_by_the_check(built):
    """pairs 61 308 .. 61 310 of the benchmark's 1 kbp batch: under wf-adaptive the ops of the middle one consume one base more than
    both sequences hold (tests/test_diff_abi.py)"""
    import wfa_amd
    from oracle import oracle as O
    from wfa_amd import _lib
    blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs(seed=3, n_pairs=3, length=1000, error_rate=0.05, first_index=61308)
    w = O.align_batch(O.make_params(global_alignment=True, adaptive=(10, 50, 1)), blob, q_off, q_len, t_off, t_len)
    br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions, w.ops_off,
                             w.ops_len, w.ops)
    a = X.from_results(w, (blob, q_off, q_len, t_off, t_len))
    assert P.restate(a, 0, len(blob), 0) is None
    with pytest.raises(_lib.WfaHipError) as ei:
        wfa_amd.pileup(br, blob, q_off, q_len, t_off, t_len, 0, len(blob))
    assert ei.value.code == _lib.ERR_BAD_ARG
    want, piled = P.restate(a, 0, len(blob), 1)
    assert piled == 3 and np.array_equal(wfa_amd.pileup(br, blob, q_off, q_len, t_off, t_len, 0, len(blob), only_aligned=True), want)
    # d_pass under WFAHIP_CHK_NO_ROWS as the status: the pair is set aside, the other two pile
    _, passed, flagged = wfa_amd.check_alignments(br, blob, q_off, q_len, t_off, t_len, mask=wfa_amd.CHK_NO_ROWS)
    assert flagged == 1 and passed.tolist() == [0, wfa_amd.PAIR_CHECK_FAILED, 0]
    br.status = passed
    b, aside = P.set_aside(a, 0)
    assert aside == [1] and np.array_equal(b["status"], passed)
    assert np.array_equal(wfa_amd.pileup(br, blob, q_off, q_len, t_off, t_len, 0, len(blob)), P.restate(b, 0, len(blob), 0)[0])


def test_device_entries_bad_args_without_device(built):
    from wfa_amd import _lib
    BAD = _lib.ERR_BAD_ARG
    ctx, p = C.c_void_p(1), C.c_void_p(4096)  # (everything below returns before the context -- the address 1 -- or a buffer is dereferenced)
    for f, packed in ((_lib.lib().wfahip_pileup_device, 0), (_lib.lib().wfahip_pileup_packed_device, 1)):
        piled = C.c_uint64(99)
        ok = [ctx, p, p, 8, p, 8, p, p, p, p] + [p] * packed + [1, 0, 0, 8, p, C.byref(piled), None]
        N, AT, PN, COUNTS, PILED = (x + packed for x in (10, 12, 13, 14, 15))

        def call(**kw):
            a = list(ok)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return f(*a)
        at = lambda i: "a%d" % i
        assert call(a0=None) == BAD
        for k in (1, 6, 7, 8, 9):                             # d_rec, the offset and length arrays
            assert call(**{at(k): None}) == BAD, k
        assert call(a2=None) == BAD                           # d_ops null with ops_cap > 0
        assert call(a4=None) == BAD                           # the blob or the words null with a size > 0
        assert call(**{"a4": None, at(N): 0}) == BAD          # ... whatever n_pairs is
        assert call(**{at(COUNTS): None}) == BAD              # null counters with pile_n > 0
        assert call(**{at(COUNTS): None, at(N): 0}) == BAD
        assert call(**{at(PN): (1 << 58) + 1}) == BAD
        assert call(**{at(N): 0xFFFFFFF1}) == BAD
        assert piled.value == 99
        # no pairs, or no window, touches nothing; the flags may be null
        kw = {at(k): None for k in (1, 2, 4, 6, 7, 8, 9, COUNTS)}
        kw.update({"a3": 0, "a5": 0, at(N): 0, at(PN): 0})
        if packed:
            kw["a10"] = None
        assert call(**kw) == 0 and piled.value == 0
        piled.value = 99
        assert call(**{at(PN): 0, at(COUNTS): None}) == 0 and piled.value == 0
        assert call(**{at(N): 0, at(PILED): None}) == 0
        assert call(**{at(PN): 1 << 58, at(N): 0}) == 0
