"""GPU: the pileup counted on the device (include/wfa_hip.h: wfahip_pileup_device, wfahip_pileup_packed_device;
Aligner.pileup_tensors, pileup_tensors_packed).  The kernels against the numpy restatement of tests/pile_cases.py and against the host
entries, counter for counter, with a canary row before and behind the counters, the inputs compared unchanged and the offsets of
every pair that is not OK poisoned: the synthetic set of tests/check_cases.py (op lists around 64 and 128 ops, unknown letters,
counts of 0, targets at every byte offset mod 16) -- refused as it is, the counters still their canary pattern, and counted once the
check's d_pass is copied over the status column --; one M op of 257, 1 000 and 70 000 columns under windows that start and end
inside it, tiles, a second call and a window outside the blob; 40 reads on each of 8 shared targets; real results of align_tensors
(semi-global, both values of only_aligned) and of align_tensors_packed with every second query flagged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_batches as B  # noqa: E402
import check_cases as X  # noqa: E402
import cigar_cases as K  # noqa: E402
import pile_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5EEDC0DE


def _aligner(prm, adaptive):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.Penalties(*prm[:3]), wfa_amd.Options(GlobalAlignment=bool(prm[3])), device=0)
    if adaptive:
        assert a.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    return a


@pytest.fixture(scope="module")
def aligners(built):
    made = {"global": _aligner((4, 6, 2, 1), (10, 50, 1)), "semi": _aligner((4, 6, 2, 0), (10, 50, 1))}
    yield made
    for a in made.values():
        a.close()


@pytest.fixture(scope="module")
def al(aligners):
    return aligners["global"]


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


def records_of(a):
    """device records of a dict of real results: STATUS, the windows, OPS_LEN and OPS_OFF, every other word junk"""
    rec = K.records(a["status"], a["ops_off"], a["ops_len"])
    rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5] = (np.asarray(a[k]).view(np.uint32) for k in ("tbegin", "tend", "qbegin", "qend"))
    return rec


def inputs(a):
    """rec, ops, then blob, q_off, q_len, t_off, t_len -- or words, q_woff, q_len, t_woff, t_len, q_rc"""
    return [dev(a["rec"] if "rec" in a else records_of(a)), dev(a["ops"])] + [dev(x) for x in a["seqs"]]


def from_device(rec, ops, seqs):
    """the restatement's view of records and ops that a device entry left"""
    r = rec.cpu().numpy().view(np.uint32)
    i32 = lambda k: r[:, k].copy().view(np.int32)
    return dict(status=i32(0), tbegin=i32(2), tend=i32(3), qbegin=i32(4), qend=i32(5), ops_len=r[:, 10].copy(),
                ops_off=r[:, 11].astype(np.uint64) | (r[:, 12].astype(np.uint64) << np.uint64(32)), ops=ops.cpu().numpy().view(np.uint64),
                seqs=tuple(seqs))


def buffer(n, base=None):
    """counters for a window of n bases with a canary row before and behind them: zero, or `base`"""
    import torch
    buf = np.zeros((n + 2, 8), np.uint32) if base is None else np.concatenate([np.zeros((1, 8), np.uint32), base, np.zeros((1, 8), np.uint32)])
    buf[0] = buf[-1] = CANARY
    return torch.from_numpy(buf.view(np.int32)).to("cuda:0")


def raw(al, ins, only, at, n, buf, stream=None, ops_cap=None, size=None):
    """the C entry itself -- the packed one for eight tensors, the byte one for seven -- into rows 1 .. n of buf: (return code,
    *n_piled)"""
    import torch
    from wfa_amd import _lib
    torch.cuda.synchronize()  # (the fills of the test ran on torch's stream; stream=None is the context's own)
    rec, ops, seqs = ins[:3]
    piled = C.c_uint64(12345)
    head = [al._ctx, rec.data_ptr(), ops.data_ptr(), ops.numel() if ops_cap is None else ops_cap, seqs.data_ptr(),
            seqs.numel() if size is None else size] + [t.data_ptr() for t in ins[3:7]]
    tail = [rec.shape[0], only, at, n, buf[1:].data_ptr(), C.byref(piled), stream]
    if len(ins) == 8:
        rc = _lib.lib().wfahip_pileup_packed_device(*head, ins[7].data_ptr() if ins[7] is not None else None, *tail)
    else:
        rc = _lib.lib().wfahip_pileup_device(*head, *tail)
    return rc, piled.value


def counters(buf):
    """the window's counters, the canary rows checked"""
    c = buf.cpu().numpy().view(np.uint32)
    assert (c[0] == CANARY).all() and (c[-1] == CANARY).all(), "a counter outside the window was written"
    return c[1:-1]


def same(got, want, what=""):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} counters differ, the first (base, word) {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def host(a, only, at, n, packed):
    """the host entry on the same arrays"""
    import wfa_amd
    z = np.zeros(len(a["status"]), np.uint32)
    br = wfa_amd.BatchResult(a["status"], z, a["tbegin"], a["tend"], a["qbegin"], a["qend"], z, z, z, z, a["ops_off"], a["ops_len"], a["ops"])
    if packed:
        return wfa_amd.pileup_packed(br, *a["seqs"][:5], at, n, q_rc=a["seqs"][5], only_aligned=bool(only), n_threads=4)
    return wfa_amd.pileup(br, *a["seqs"], at, n, only_aligned=bool(only), n_threads=4)


def set_aside_on_device(al, a, ins, only, packed):
    """what a caller does with a batch that holds a bad pair: the check's d_pass under NO_ROWS (NO_ROWS_TRIMMED) copied over the
    status column of a copy of the records.  Returns (the restatement's dict of the remaining pairs, the device inputs with that
    copy and with the offsets of every pair that is not OK poisoned)"""
    import wfa_amd
    mask = wfa_amd.CHK_NO_ROWS_TRIMMED if only else wfa_amd.CHK_NO_ROWS
    if packed:
        _, passed, flagged = al.check_tensors_packed(*ins[:7], q_rc=ins[7], mask=mask)
    else:
        _, passed, flagged = al.check_tensors(*ins, mask=mask)
    b, aside = P.set_aside(a, only, packed)
    assert flagged == len(aside) and np.array_equal(passed.cpu().numpy(), b["status"])
    rec2 = ins[0].clone()
    rec2[:, 0] = passed
    return b, [rec2, ins[1], ins[2]] + [dev(x) for x in b["seqs"][1:]]


def pile_and_compare(al, b, ins, only, at, n, packed, what=""):
    want, want_piled = P.restate(b, at, n, only, packed)
    buf = buffer(n)
    rc, piled = raw(al, ins, only, at, n, buf)
    assert rc == 0 and piled == want_piled, (rc, piled, want_piled)
    got = counters(buf)
    same(got, want, what)
    return got, buf


@pytest.mark.parametrize("only", [0, 1])
@pytest.mark.parametrize("packed", [False, True])
def test_synthetic_set(al, packed, only):
    import torch
    from wfa_amd import _lib
    cs = X.cases()
    assert {len(c["ops"]) for c in cs} >= {63, 64, 65, 128, 129, 200} and any(n == 70001 for c in cs for _, n in X.split(c["ops"]))
    a = X.arrays(cs, packed=packed, flags=[i & 1 for i in range(len(cs))] if packed else None, junk_tails=9 if packed else None)
    ins = inputs(a)
    before = [t.clone() for t in ins]
    at, n = P.span(a, packed)
    # a batch with a bad pair: WFAHIP_ERR_BAD_ARG, every counter still the pattern it held
    pattern = np.random.default_rng(1).integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    buf = buffer(n, pattern)
    rc, piled = raw(al, ins, only, at, n, buf)
    assert rc == _lib.ERR_BAD_ARG and np.array_equal(counters(buf), pattern)
    # ... and counted once d_pass is copied over the status column; the offsets of the pairs that are not OK are poison
    b, ins2 = set_aside_on_device(al, a, ins, only, packed)
    got, _ = pile_and_compare(al, b, ins2, only, at, n, packed)
    assert got.any()
    same(got, host(b, only, at, n, packed), "host")
    rc, piled = raw(al, ins2, only, at, n, buf)                   # the entries add: on top of the pattern, wrapping
    assert rc == 0
    same(counters(buf), P.restate(b, at, n, only, packed, into=pattern)[0], "added")
    assert all(torch.equal(x, y) for x, y in zip(ins, before))    # the inputs are only read


def _long_cases():
    rng = np.random.default_rng(77)
    op = X.op
    return [X.clean("257", [op("M", 257)], rng), X.clean("1000", [op("D", 2), op("M", 1000), op("I", 3)], rng),
            X.clean("70000", [op("X", 1), op("M", 70000), op("D", 5)], rng), X.clean("long gap", [op("M", 3), op("I", 70000), op("M", 2)], rng)]


@pytest.mark.parametrize("packed", [False, True])
def test_one_long_op_windows_tiles_and_a_second_call(al, packed):
    cs = _long_cases()
    a = X.arrays(cs, packed=packed, flags=[0, 1, 1, 0] if packed else None)
    if not packed:                                                # one byte in front: every target at an odd byte offset
        blob, q_off, q_len, t_off, t_len = a["seqs"]
        a["seqs"] = (np.concatenate([np.array([7], np.uint8), blob]), q_off + np.uint64(1), q_len, t_off + np.uint64(1), t_len)
        assert all(int(o) & 1 for o in a["seqs"][3])
    ins = inputs(a)
    t_off, t_len = a["seqs"][3], a["seqs"][4]
    coord = lambda i, p: (16 if packed else 1) * int(t_off[i]) + p
    at, n = P.span(a, packed)
    whole, _ = pile_and_compare(al, a, ins, 0, at, n, packed)
    same(whole, host(a, 0, at, n, packed), "host")
    for i in range(4):                                            # every base of a target is covered once
        assert (whole[coord(i, 0):coord(i, int(t_len[i])), :6].sum(axis=1) == 1).all()
    # windows that start and end inside the one long op
    for i, p, k in ((0, 100, 57), (1, 1, 997), (2, 12345, 40001), (3, 64, 64), (2, 69999, 2)):
        part, buf = pile_and_compare(al, a, ins, 0, coord(i, p), k, packed, f"window {i}")
        same(part, whole[coord(i, p):coord(i, p) + k])
        rc, _ = raw(al, ins, 0, coord(i, p), k, buf)              # a second call doubles the counters
        assert rc == 0
        same(counters(buf), 2 * part, f"second call {i}")
    # two tiles whose concatenation is the full window, the cut inside the 70 000 columns
    cut = coord(2, 33333)
    left, _ = pile_and_compare(al, a, ins, 0, at, cut - at, packed)
    right, _ = pile_and_compare(al, a, ins, 0, cut, at + n - cut, packed)
    same(np.concatenate([left, right]), whole, "tiles")
    # a window outside the blob (the words) receives nothing; every pair is still swept
    for far in (at + n + 7, (1 << 64) - 4096):
        buf = buffer(64)
        rc, piled = raw(al, ins, 0, far, 64, buf)
        assert rc == 0 and piled == 4 and not counters(buf).any()


@pytest.mark.parametrize("only", [0, 1])
@pytest.mark.parametrize("packed", [False, True])
def test_depth_40_on_shared_targets(al, packed, only):
    """t_off repeated: the adds of 40 waves meet on every base of a target and sum exactly"""
    S = P.shared_targets()
    a = S["words" if packed else "bytes"]
    ins = inputs(a)
    at, n = P.span(a, packed)
    got, _ = pile_and_compare(al, a, ins, only, at, n, packed)
    same(got, host(a, only, at, n, packed), "host")
    for to, tw, tl in S["targets"]:
        c = 16 * tw if packed else to
        if only == 0:
            assert (got[c:c + tl, :6].sum(axis=1) == S["depth"]).all()
        assert got[c:c + tl, :6].sum() >= (tl - 20) * S["depth"]
    to, tw, tl = S["targets"][5]
    c = 16 * tw if packed else to
    part, _ = pile_and_compare(al, a, ins, only, c + 33, 200, packed)
    same(part, got[c + 33:c + 233])


def _align_and_pile(al, ins_seqs, seqs_np, packed, only, q_rc=None):
    """align on the device, set the pairs the check flags aside, pile over everything, compare"""
    import torch
    if packed:
        rec, ops = al.align_tensors_packed(*ins_seqs, q_rc=q_rc)
        ins = [rec, ops] + list(ins_seqs) + [q_rc]
    else:
        rec, ops = al.align_tensors(*ins_seqs)
        ins = [rec, ops] + list(ins_seqs)
    a = from_device(rec, ops, seqs_np)
    before = [t.clone() for t in ins]
    b, ins2 = set_aside_on_device(al, a, ins, only, packed)
    at, n = P.span(a, packed)
    got, _ = pile_and_compare(al, b, ins2, only, at, n, packed)
    same(got, host(b, only, at, n, packed), "host")
    assert all(torch.equal(x, y) for x, y in zip(ins, before))
    return a, b, ins2, got


@pytest.mark.parametrize("only", [0, 1])
def test_real_results_semi_global(aligners, only):
    """align_tensors' records and ops of the semi-global batch (targets with overhangs), both values of only_aligned"""
    seqs = B.batch("semi-global 200")["seqs"]
    a, b, ins2, got = _align_and_pile(aligners["semi"], [dev(x) for x in seqs], seqs, False, only)
    assert (b["status"] == 0).sum() >= len(b["status"]) - 3
    if only:  # trimmed, an alignment covers [TBEGIN - 1, TEND) of its target once
        for i in range(0, len(b["status"]), 37):
            if b["status"][i] == 0:
                to, lo, hi = int(seqs[3][i]), int(b["tbegin"][i]) - 1, int(b["tend"][i])
                assert (got[to + lo:to + hi, :6].sum(axis=1) == 1).all() and not got[to:to + lo, :6].any()


def test_real_results_packed_both_strands_and_the_wrappers(al):
    """pack_tensors -> align_tensors_packed with every second query flagged -> pileup_tensors_packed; then the byte entry on the same
    forward pairs: base p of the sequence at word w is 16 w + p"""
    import torch
    seqs = B.batch("global 300")["seqs"]
    k = 600
    seqs = (seqs[0],) + tuple(x[:k] for x in seqs[1:])
    d = [dev(x) for x in seqs]
    packed, q_woff, t_woff = al.pack_tensors(*d)
    q_rc = dev((np.arange(k) & 1).astype(np.uint8))
    pk_np = (packed.cpu().numpy().view(np.uint32), q_woff.cpu().numpy().view(np.uint64), seqs[2], t_woff.cpu().numpy().view(np.uint64), seqs[4],
             q_rc.cpu().numpy())
    a, b, ins2, got = _align_and_pile(al, [packed, q_woff, d[2], t_woff, d[4]], pk_np, True, 1, q_rc=q_rc)
    assert not got[:, P.OTHER].any()
    k_piled = int((b["status"] == 0).sum())                       # (an OK pair of this batch has a column)
    assert k_piled >= k - 8
    # the wrapper: a zeroed tensor without out=, accumulation with it, n_piled, a caller-owned stream
    at, n = P.span(a, True)
    counts, piled = al.pileup_tensors_packed(*ins2[:7], at, n, q_rc=q_rc, only_aligned=True)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (n, 8) and piled == k_piled
    same(counts.cpu().numpy().view(np.uint32), got)
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        again, piled = al.pileup_tensors_packed(*ins2[:7], at, n, q_rc=q_rc, only_aligned=True, out=counts, stream=s)
    s.synchronize()
    assert again is counts and piled == k_piled
    same(counts.cpu().numpy().view(np.uint32), 2 * got)
    # forward pairs from bytes and from words, position for position
    rec, ops = al.align_tensors(*d)
    by, n_by = al.pileup_tensors(rec, ops, *d, 0, seqs[0].size, only_aligned=True)
    rec_pk, ops_pk = al.align_tensors_packed(packed, q_woff, d[2], t_woff, d[4])
    pk, n_pk = al.pileup_tensors_packed(rec_pk, ops_pk, packed, q_woff, d[2], t_woff, d[4], 0, 16 * packed.numel(), only_aligned=True)
    assert n_by == n_pk == k
    by, pk, tw = by.cpu().numpy(), pk.cpu().numpy(), pk_np[3]
    for i in range(0, k, 11):
        to, tl = int(seqs[3][i]), int(seqs[4][i])
        assert np.array_equal(by[to:to + tl], pk[16 * int(tw[i]):16 * int(tw[i]) + tl]), i
    want, _ = P.restate(from_device(rec, ops, seqs), 0, seqs[0].size, 1)
    same(by.view(np.uint32), want, "bytes")
    with pytest.raises(ValueError):
        al.pileup_tensors(rec, ops, *d, 0, 8, out=torch.zeros((9, 8), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        al.pileup_tensors(rec, ops, *d, 0, 8, out=torch.zeros((8, 8), dtype=torch.int64, device="cuda:0"))
    empty, piled = al.pileup_tensors(rec, ops, *d, 5, 0)
    assert tuple(empty.shape) == (0, 8) and piled == 0


@pytest.mark.parametrize("packed", [False, True])
def test_checks_before_the_kernel_that_reads_a_sequence(al, packed):
    """one clean pair: the blob (the words) one short of the later sequence's end, an op range one past the op buffer, a trimmed window
    one base too small -- each WFAHIP_ERR_BAD_ARG with the counters untouched, next to the same input at its bound"""
    from wfa_amd import _lib
    c = X.cases()[0]
    a = X.arrays([c], packed=packed, flags=[1] if packed else None)
    ins = inputs(a)
    at, n = P.span(a, packed)
    size, ops_end = len(a["seqs"][0]), int(a["ops_off"][0] + a["ops_len"][0])
    for only in (0, 1):
        for kw in (dict(size=size - 1), dict(ops_cap=ops_end - 1), dict(size=0)):
            buf = buffer(n)
            rc, piled = raw(al, ins, only, at, n, buf, **kw)
            assert rc == _lib.ERR_BAD_ARG and not counters(buf).any(), kw
        buf = buffer(n)
        rc, piled = raw(al, ins, only, at, n, buf, size=size, ops_cap=ops_end)   # both end exactly at their bounds
        assert rc == 0 and piled == 1
        same(counters(buf), P.restate(a, at, n, only, packed)[0])
    short = dict(a, rec=a["rec"].copy(), qend=a["qend"] - 1)
    short["rec"][:, 5] -= 1
    assert P.restate(short, at, n, 1, packed) is None
    buf = buffer(n)
    rc, piled = raw(al, inputs(short), 1, at, n, buf)
    assert rc == _lib.ERR_BAD_ARG and not counters(buf).any()
    rc, piled = raw(al, inputs(short), 0, at, n, buf)                            # untrimmed the record's window is not looked at
    assert rc == 0 and piled == 1
