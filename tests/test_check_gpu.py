"""GPU: the check on the device (include/wfa_hip.h: wfahip_check_alignments_device, wfahip_check_alignments_packed_device;
Aligner.check_tensors, check_tensors_packed).  The kernels against the host entries and the restatement of tests/check_cases.py:
the synthetic set over bytes and over words of both strands under four masks, with canaries behind the outputs and the inputs
unchanged; the shapes at which a wave per pair in rounds of 64 ops can go wrong; real results of align_tensors and
align_tensors_packed against the host check of the oracle's; real results tampered with; and the contract with the text entries and
wfahip_select_pairs_device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_batches as B  # noqa: E402
import check_cases as X  # noqa: E402
from check_cases import op  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = 0x5EEDBEEF
PRMS = {"global": X.PARAMS, "semi-global": X.PARAMS[:3] + (0,), "huge-penalties": X.HUGE}


def _aligner(prm, adaptive=None):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.Penalties(*prm[:3]), wfa_amd.Options(GlobalAlignment=bool(prm[3])), device=0)
    if adaptive:
        assert a.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    return a


@pytest.fixture(scope="module")
def aligners(built):
    made = {k: _aligner(p) for k, p in PRMS.items()}
    yield made
    for a in made.values():
        a.close()


@pytest.fixture(scope="module")
def al(aligners):
    return aligners["global"]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


def _inputs(a):
    """check_cases.arrays' dict as the device tensors of the entry: rec, ops, blob or words, q_off, q_len, t_off, t_len[, q_rc]"""
    return [_dev(a["rec"]), _dev(a["ops"])] + [_dev(x) for x in a["seqs"]]


def _check(al, ins, packed, mask=X.ALL):
    """the method into canaried outputs: (chk uint32 [n, 8], passed int32 [n], n_flagged); nothing behind them is written"""
    import torch
    n = ins[0].shape[0]
    chk = torch.full((n + 2, 8), CANARY, dtype=torch.int32, device="cuda:0")
    passed = torch.full((n + 5,), CANARY, dtype=torch.int32, device="cuda:0")
    f = al.check_tensors_packed if packed else al.check_tensors
    kw = dict(q_rc=ins[7]) if packed else {}
    out = f(*ins[:7], mask=mask, out=(chk[:n], passed[:n]), **kw)
    assert out[0].data_ptr() == chk.data_ptr() and out[1].data_ptr() == passed.data_ptr()
    assert (chk[n:] == CANARY).all() and (passed[n:] == CANARY).all()
    return chk[:n].cpu().numpy().view(np.uint32), passed[:n].cpu().numpy(), out[2]


def _same(got, want, names=None):
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{bad.size} pairs differ; first {i} {names[i] if names else ''}: got {list(got[i])} "
                             f"{sorted(X.names_of(int(got[i][0])))}, want {list(want[i])} {sorted(X.names_of(int(want[i][0])))}")


def _host(a, prm, packed=False, mask=X.ALL):
    import wfa_amd
    br = wfa_amd.BatchResult(a["status"], a["score"], a["tbegin"], a["tend"], a["qbegin"], a["qend"], a["align_len"], a["matches"], a["gaps"],
                             a["gap_regions"], a["ops_off"], a["ops_len"], a["ops"])
    f = wfa_amd.check_alignments_packed if packed else wfa_amd.check_alignments
    return f(br, *a["seqs"], penalties=wfa_amd.Penalties(*prm[:3]), options=wfa_amd.Options(GlobalAlignment=bool(prm[3])), mask=mask)


MASKS = [X.ALL, X.BIT["NO_ROWS"], 0, X.BIT["M_DIFFERS"] | X.BIT["COST_UNDER"]]


# ---- 1. the synthetic set

@pytest.mark.parametrize("layout", ["bytes", "words", "words-all-flagged", "words-alt-junk"])
@pytest.mark.parametrize("prm", list(PRMS))
def test_synthetic_set(aligners, prm, layout):
    import torch
    cases = X.cases()
    n = len(cases)
    packed = layout != "bytes"
    flags = {"bytes": None, "words": [0] * n, "words-all-flagged": [1] * n, "words-alt-junk": [i & 1 for i in range(n)]}[layout]
    a = X.arrays(cases, packed=packed, flags=flags, junk_tails=9 if layout == "words-alt-junk" else None)
    want = X.restate(a, PRMS[prm], packed=packed)
    ins = _inputs(a)
    before = [t.clone() for t in ins]
    for mask in MASKS:
        chk, passed, n_flagged = _check(aligners[prm], ins, packed, mask)
        _same(chk, want, [c["name"] for c in cases])
        h_chk, h_passed, h_n = _host(a, PRMS[prm], packed, mask)
        assert np.array_equal(chk, h_chk) and np.array_equal(passed, h_passed) and n_flagged == h_n
        want_pass, want_n = X.passed_of(a["status"], want, mask)
        assert np.array_equal(passed, want_pass) and n_flagged == want_n
    assert all(torch.equal(x, y) for x, y in zip(ins, before))  # the inputs are only read
    # out=None, and q_rc=None for no flags; an output that is not 16-byte aligned takes the word stores
    al = aligners[prm]
    f = al.check_tensors_packed if packed else al.check_tensors
    c2, p2, n2 = f(*ins[:7]) if layout in ("bytes", "words") else f(*ins[:7], q_rc=ins[7])
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), want) and n2 == X.passed_of(a["status"], want, X.ALL)[1]
    odd = torch.full((n * 8 + 9,), CANARY, dtype=torch.int32, device="cuda:0")
    view = odd[1:1 + 8 * n].view(n, 8)
    assert view.data_ptr() % 16 == 4
    f(*ins[:7], out=(view, p2), **(dict(q_rc=ins[7]) if packed else {}))
    assert np.array_equal(view.cpu().numpy().view(np.uint32), want) and odd[0] == CANARY and (odd[1 + 8 * n:] == CANARY).all()


# ---- 2. shapes

def _mx_case(name, n_ops, rng):
    """ops that alternate M and X: every column is compared, and column c reads query base c and target base c"""
    return X.clean(name, [op("MX"[k & 1], int(rng.integers(1, 9))) for k in range(n_ops)], rng)


def _bad_at(case, c, name):
    """the case with column c made bad: a base flipped under an M column, the target's base copied under an X column"""
    ends = np.cumsum([n for _, n in X.split(case["ops"])])
    is_m = (int(case["ops"][int(np.searchsorted(ends, c, side="right"))]) >> 32) == ord("M")
    if is_m:
        return X.changed(case, name, ["M_DIFFERS"], q=X.flip(case["q"], c))
    return X.changed(case, name, ["X_EQUAL"], t=case["t"][:c] + case["q"][c:c + 1] + case["t"][c + 1:])


def test_bad_columns_at_every_seam(al):
    """one bad column each at the first and the last column, at the last column of a round of 64 ops and the first of the next, at
    the first and the last column of a lane's group of four and of a sweep of 256; in a pair of three rounds and in one op of
    70 001 columns.  FIRST_BAD names the column, N_BAD is 1."""
    rng = np.random.default_rng(77)
    multi = _mx_case("130 ops", 130, rng)
    ends = np.cumsum([n for _, n in X.split(multi["ops"])])
    total = int(ends[-1])
    at = [0, total - 1, int(ends[63]) - 1, int(ends[63]), int(ends[127]) - 1, int(ends[127]), 8, 11, 255, 256]
    long_ = X.clean("long", [op("M", 70001)], rng)
    at_long = [0, 70000, 255, 256, 4 * 9000, 4 * 9000 + 3, 69999, 65535, 65536]
    cases = [multi, long_] + [_bad_at(multi, c, f"multi {c}") for c in at] + [_bad_at(long_, c, f"long {c}") for c in at_long]
    cols = [None, None] + at + at_long
    for packed in (False, True):
        a = X.arrays(cases, packed=packed, flags=[i & 1 for i in range(len(cases))])
        chk, _, n_flagged = _check(al, _inputs(a), packed)
        _same(chk, X.restate(a, X.PARAMS, packed=packed), [c["name"] for c in cases])
        for c, w, col in zip(cases, chk, cols):
            assert X.names_of(int(w[0])) == c["claims"], c["name"]
            assert (int(w[4]), int(w[5])) == ((0, X.NONE) if col is None else (1, col)), c["name"]
        assert n_flagged == len(cases) - 2


@pytest.mark.parametrize("n", [1, 3, 257])
def test_number_of_pairs_and_of_ops(al, n):
    """1, 3 and 257 pairs (a workgroup that is not full, and more than one); op lists of 0, 1, 63, 64, 65, 128, 129 and 200 ops; one op of 70 001 columns; UNMERGED across the seam of two rounds"""
    rng = np.random.default_rng(5)
    seam = [op("MX"[(k + (k >= 64)) & 1], 2) for k in range(130)]  # ops 63 and 64, and no others, are both X: that neighbour compare spans two rounds
    no_seam = [op("MX"[k & 1], 2) for k in range(130)]
    named = {c["name"]: c for c in X.cases()}
    pool = [named[f"{k} ops"] for k in X.N_OPS[1:]] + [named["empty"], named["70000 columns"], X.clean("seam", seam, rng, ["UNMERGED"]),
                                                      X.clean("no seam", no_seam, rng), named["m differs and x equal"], named["status 4"]]
    cases = [pool[(i + n) % len(pool)] for i in range(n)]
    if n == 257:
        assert all(any(c is p for c in cases) for p in pool)
    for packed in (False, True):
        a = X.arrays(cases, packed=packed, flags=[(i >> 1) & 1 for i in range(n)], seed=n)
        want = X.restate(a, X.PARAMS, packed=packed)
        chk, passed, n_flagged = _check(al, _inputs(a), packed)
        _same(chk, want, [c["name"] for c in cases])
        for c, w in zip(cases, want):
            assert X.names_of(int(w[0])) == c["claims"], c["name"]
        want_pass, want_n = X.passed_of(a["status"], want, X.ALL)
        assert np.array_equal(passed, want_pass) and n_flagged == want_n


def test_empty_batch_and_null_outputs(al):
    import ctypes as C
    import torch
    from wfa_amd import _lib
    z = lambda dt, shape=0: torch.zeros(shape, dtype=dt, device="cuda:0")
    chk, passed, n = al.check_tensors(z(torch.int32, (0, 16)), z(torch.int64), z(torch.uint8), z(torch.int64), z(torch.int32), z(torch.int64),
                                      z(torch.int32))
    assert chk.shape == (0, 8) and passed.numel() == 0 and n == 0
    # d_pass and n_flagged may be null
    a = X.arrays(list(X.cases()[:6]))
    ins = _inputs(a)
    out = torch.full((6, 8), CANARY, dtype=torch.int32, device="cuda:0")
    prm = _lib.Params(4, 6, 2, 1, 0)
    torch.cuda.synchronize()
    rc = _lib.lib().wfahip_check_alignments_device(al._ctx, C.byref(prm), ins[0].data_ptr(), ins[1].data_ptr(), ins[1].numel(), ins[2].data_ptr(),
                                                   ins[2].numel(), *[t.data_ptr() for t in ins[3:7]], 6, X.ALL, out.data_ptr(), None, None, None)
    assert rc == 0 and np.array_equal(out.cpu().numpy().view(np.uint32), X.restate(a, X.PARAMS))


def test_caller_owned_stream(al):
    import torch
    a = X.arrays(list(X.cases()))
    ins = _inputs(a)
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    chk, passed, n = al.check_tensors(*ins[:7], stream=s)
    assert np.array_equal(chk.cpu().numpy().view(np.uint32), X.restate(a, X.PARAMS))


# ---- 3. real results

def _blob_to_device(seqs, pad=64):
    blob, q_off, q_len, t_off, t_len = seqs
    return (_dev(np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(pad, np.uint8)])), _dev(np.asarray(q_off, np.uint64)),
            _dev(np.asarray(q_len, np.uint32)), _dev(np.asarray(t_off, np.uint64)), _dev(np.asarray(t_len, np.uint32)))


def _host_of_oracle(b, packed=False):
    import wfa_amd
    w = b["oracle"]
    br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions, w.ops_off,
                             w.ops_len, w.ops)
    kw = dict(penalties=wfa_amd.Penalties(*b["prm"][:3]), options=wfa_amd.Options(GlobalAlignment=bool(b["prm"][3])))
    if packed:
        return wfa_amd.check_alignments_packed(br, *B.packed(b), **kw)
    return wfa_amd.check_alignments(br, *b["seqs"], **kw)


@pytest.mark.parametrize("name", list(B.SPEC))
def test_real_results_equal_the_host_check_of_the_oracles(built, name):
    """align_tensors / align_tensors_packed (every second pair flagged) -> check_tensors / check_tensors_packed, against
    wfahip_check_alignments over the oracle's results for the same input: the ops lie elsewhere, the verdicts are the same"""
    b = B.batch(name)
    a = _aligner(b["prm"], b["adaptive"])
    try:
        d = _blob_to_device(b["seqs"])
        rec, ops = a.align_tensors(*d)
        blob = d[0][:len(b["seqs"][0])]                            # (the check needs nothing behind the last sequence)
        chk, passed, n_flagged = _check(a, [rec, ops, blob, *d[1:]], False)
        words, q_woff, q_len, t_woff, t_len, q_rc = (_dev(x) for x in B.packed(b))
        import torch
        slack = torch.cat([words, torch.zeros(4, dtype=torch.int32, device="cuda:0")])
        rec_pk, ops_pk = a.align_tensors_packed(slack, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
        chk_pk, passed_pk, n_pk = _check(a, [rec_pk, ops_pk, words, q_woff, q_len, t_woff, t_len, q_rc], True)
    finally:
        a.close()
    h_chk, h_passed, h_n = _host_of_oracle(b)
    _same(chk, h_chk)
    assert np.array_equal(passed, h_passed) and n_flagged == h_n
    p_chk, p_passed, p_n = _host_of_oracle(b, packed=True)
    _same(chk_pk, p_chk)
    assert np.array_equal(passed_pk, p_passed) and n_pk == p_n
    if name == "aggressive":
        count = {n: int(((chk[:, 0] & X.BIT[n]) != 0).sum()) for n in X.NAMES}
        assert count["M_DIFFERS"] >= 1 and count["Q_OVER"] + count["T_OVER"] >= 1 and count["COST_UNDER"] >= 1 and n_flagged > 0
    else:
        assert n_flagged == 0 and not chk[:, 0].any() and n_pk == 0


# ---- 4. real results, tampered with

def test_tampering_lands_on_its_pair_as_its_flags(al):
    import torch
    b = B.batch("global 300")
    d = _blob_to_device(b["seqs"])
    rec, ops = al.align_tensors(*d)
    base, _, n0 = _check(al, [rec, ops, *d], False)
    assert n0 == 0 and not base[:, 0].any()
    R, O_ = rec.cpu().numpy().view(np.uint32).copy(), ops.cpu().numpy().view(np.uint64).copy()
    blob = d[0].cpu().numpy().copy()
    q_off, q_len = b["seqs"][1], b["seqs"][2]
    pair_ops = lambda i: O_[(int(R[i, 11]) | int(R[i, 12]) << 32):][:int(R[i, 10])]
    letters = lambda i: [int(o) >> 32 for o in pair_ops(i)]
    used, want = set(), {}

    def pick(ok):
        i = next(i for i in range(len(R)) if i not in used and ok(i))
        used.add(i)
        return i, (int(R[i, 11]) | int(R[i, 12]) << 32)
    inner_x = lambda i: next((k for k in range(1, len(letters(i)) - 1) if letters(i)[k - 1:k + 2] == [77, 88, 77]), None)
    # an X between two Ms becomes an M: its neighbours are of its letter, its columns differ, the CIGAR is cheaper, more matches
    i, off = pick(lambda i: inner_x(i) is not None)
    O_[off + inner_x(i)] = (ord("M") << 32) | (int(O_[off + inner_x(i)]) & X.M32)
    want[i] = {"UNMERGED", "M_DIFFERS", "COST_UNDER", "STAT_MATCHES"}
    # one base of the blob under an M column: the first op is an M of at least 3 columns
    i, off = pick(lambda i: letters(i)[0] == 77 and int(pair_ops(i)[0]) & X.M32 >= 3)
    blob[int(q_off[i]) + 2] = ord(X.flip(bytes(blob[int(q_off[i]) + 2:int(q_off[i]) + 3]), 0))
    want[i] = {"M_DIFFERS"}
    first_bad = i
    # the count of the last op, an M, one more and one less
    i, off = pick(lambda i: letters(i)[-1] == 77 and int(pair_ops(i)[-1]) & X.M32 >= 2)
    O_[off + len(letters(i)) - 1] += np.uint64(1)
    want[i] = {"Q_OVER", "T_OVER", "NO_ROWS", "NO_ROWS_TRIMMED", "STAT_ALIGN_LEN", "STAT_MATCHES"}
    i, off = pick(lambda i: letters(i)[-1] == 77 and int(pair_ops(i)[-1]) & X.M32 >= 2)
    O_[off + len(letters(i)) - 1] -= np.uint64(1)
    want[i] = {"Q_UNDER", "T_UNDER", "STAT_ALIGN_LEN", "STAT_MATCHES"}
    # the score, two more and two less
    i, _ = pick(lambda i: R[i, 1] >= 2)
    R[i, 1] += 2
    want[i] = {"COST_UNDER"}
    i, _ = pick(lambda i: R[i, 1] >= 2)
    R[i, 1] -= 2
    want[i] = {"COST_OVER"}
    # a statistic
    i, _ = pick(lambda i: True)
    R[i, 8] += 1
    want[i] = {"STAT_GAPS"}
    chk, passed, n_flagged = _check(al, [_dev(R), _dev(O_), _dev(blob), *d[1:]], False)
    for i in range(len(R)):
        if i in want:
            assert X.names_of(int(chk[i, 0])) == want[i], (i, sorted(X.names_of(int(chk[i, 0]))))
        else:
            assert np.array_equal(chk[i], base[i]), i
    assert n_flagged == len(want) == 7 and sorted(np.flatnonzero(passed == X.CHECK_FAILED)) == sorted(want)
    assert (int(chk[first_bad, 4]), int(chk[first_bad, 5])) == (1, 2)
    a = dict(status=R[:, 0].astype(np.int32), score=R[:, 1], tbegin=R[:, 2].view(np.int32), tend=R[:, 3].view(np.int32), qbegin=R[:, 4].view(np.int32),
             qend=R[:, 5].view(np.int32), align_len=R[:, 6], matches=R[:, 7], gaps=R[:, 8], gap_regions=R[:, 9], ops_len=R[:, 10],
             ops_off=R[:, 11].astype(np.uint64) | (R[:, 12].astype(np.uint64) << np.uint64(32)), ops=O_,
             seqs=(blob[:len(b["seqs"][0])],) + tuple(b["seqs"][1:]))
    _same(chk, X.restate(a, X.PARAMS))


# ---- 5. the contract with the text entries and the selection

@pytest.mark.parametrize("only", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_set_aside_pairs_let_the_text_entries_render_the_rest(al, packed, only):
    import wfa_amd
    from wfa_amd import _lib
    cases = list(X.cases())
    n = len(cases)
    a = X.arrays(cases, packed=packed, flags=[i & 1 for i in range(n)])
    ins = _inputs(a)
    flag = X.BIT["NO_ROWS_TRIMMED" if only else "NO_ROWS"]
    text = al.alignment_text_tensors_packed if packed else al.alignment_text_tensors
    kw = dict(q_rc=ins[7]) if packed else {}
    chk, passed, n_flagged = _check(al, ins, packed, flag)
    assert 3 < n_flagged < n and n_flagged == int(((chk[:, 0] & flag) != 0).sum())
    # a batch in which some pair has the flag is refused; one of the pairs without it is not
    with pytest.raises(_lib.WfaHipError) as ei:
        text(*ins[:7], only_aligned=only, **kw)
    assert ei.value.code == _lib.ERR_BAD_ARG
    keep = [i for i in range(n) if not chk[i, 0] & flag]
    b = X.arrays([cases[i] for i in keep], packed=packed, flags=[i & 1 for i in keep])
    sub = _inputs(b)
    text(*sub[:7], only_aligned=only, **(dict(q_rc=sub[7]) if packed else {}))
    # d_pass over the records' status column: the rest renders, as the host renderer renders it
    rec = ins[0].clone()
    rec[:, 0] = _dev(passed)
    rows = text(rec, *ins[1:7], only_aligned=only, **kw)
    br = wfa_amd.BatchResult(passed, a["score"], a["tbegin"], a["tend"], a["qbegin"], a["qend"], a["align_len"], a["matches"], a["gaps"],
                             a["gap_regions"], a["ops_off"], a["ops_len"], a["ops"])
    host = (wfa_amd.alignment_text_packed if packed else wfa_amd.alignment_text)(br, *a["seqs"], only_aligned=only)
    for h, g in zip(host, rows):
        assert np.array_equal(g.cpu().numpy().view(h.dtype), h)
    assert int(host[3][-1]) > 70000
    # d_pass is wfahip_select_pairs_device's d_status: exactly the unflagged OK pairs
    idx = al.select_tensors(_dev(passed), *ins[3:7])[0]
    assert list(idx.cpu().numpy()) == [i for i in range(n) if a["status"][i] == X.OK and not chk[i, 0] & flag]
