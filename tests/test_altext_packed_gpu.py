"""GPU: the display rows rendered on the device from 2-bit packed words, both strands (include/wfa_hip.h:
wfahip_alignment_text_packed_device; Aligner.alignment_text_tensors_packed).  The kernels on the synthetic records and ops of
tests/altext_cases.py over ACGT sequences packed by tests/altext_pk_cases.py -- a flagged query stored as its reverse complement --
against AlignmentResult.AlignmentText, byte for byte, with everything behind the rows still poisoned and the inputs unchanged: every
seam of the words, the groups, the sweeps and the rounds on both strands, trimmed windows at every residue of a word, ops that make
the groups cross op boundaries, sequences that share words, random tail bits and pad words; the capacity and validation errors, each
next to the same record at the bound; a caller-owned stream; and end to end behind pack_tensors and align_tensors_packed, against
the byte entry on the reverse-complemented bytes and against the oracle.  No test hands the write kernel anything the length kernel
has not accepted."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import altext_cases as A  # noqa: E402
import altext_pk_cases as P  # noqa: E402
import cigar_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
POISON = 0xA5
SCAN_BLOCK_PAIRS = 4096  # wfa_cigar.hip: CIG_SCAN_BLOCK * CIG_SCAN_ITEMS
FLAGS = ["none", "all", "alt"]


@pytest.fixture(scope="module")
def al(built):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=True), device=0)
    yield a
    a.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).to("cuda:0")


def _inputs(a):
    """altext_pk_cases.arrays' dict as the eight device tensors of the entry: rec, ops, words, q_woff, q_len, t_woff, t_len, q_rc"""
    rec = A.records(a["status"], a["ops_off"], a["ops_len"], a["win"])
    return [_dev(rec), _dev(a["ops"])] + [_dev(x) for x in a["pk"]]


def _manual(cases, pk, seed=9):
    """arrays for cases whose words the test lays out itself"""
    status, ops_off, ops_len, ops = K.lay_out([c[:2] for c in cases], seed=seed)
    return dict(status=status, ops_off=ops_off, ops_len=ops_len, ops=ops, win=A.windows(cases), pk=pk)


@functools.lru_cache(maxsize=None)
def _synthetic(n):
    """test_altext_gpu.py's pick of n cases -- the multi-round, moved-window and long-op pairs first; past the set the pairs of up
    to 1 025 columns repeat -- over ACGT, with both expected results (they do not depend on the flags: a case's query bytes are the
    strand its record speaks of)"""
    cases = P.with_acgt(A.cases())
    ops_n = lambda c: len(c[1] or [])
    first = [c for c in cases if ops_n(c) == 200][:1] + [c for c in cases if A.consumed(c[1] or [])[0] > 5000]
    first += [c for c in cases if ops_n(c) in (65, 129)]
    pool = first + [c for c in cases if not any(c is f for f in first)]
    small = [c for c in pool if A.consumed(c[1] or [])[0] <= 1025]
    picked = pool[:n] + [small[i % len(small)] for i in range(max(0, n - len(pool)))]
    return picked, A.expected(picked, 0), A.expected(picked, 1)


def _raw(al, ins, only, planes, row_cap, off, stream=None, ops_cap=None, n_words=None):
    """the C entry itself: (return code, *row_needed)"""
    import torch
    from wfa_amd import _lib
    torch.cuda.synchronize()  # (the fills of the test ran on torch's stream; stream=None is the context's own)
    rec, ops, words, q_woff, q_len, t_woff, t_len, q_rc = ins
    need = C.c_uint64(12345)
    ptrs = [p.data_ptr() if p is not None else None for p in planes]
    rc = _lib.lib().wfahip_alignment_text_packed_device(
        al._ctx, rec.data_ptr(), ops.data_ptr(), ops.numel() if ops_cap is None else ops_cap, words.data_ptr(),
        words.numel() if n_words is None else n_words, q_woff.data_ptr(), q_len.data_ptr(), t_woff.data_ptr(), t_len.data_ptr(),
        q_rc.data_ptr() if q_rc is not None else None, rec.shape[0], only, *ptrs, row_cap, off.data_ptr(), C.byref(need), stream)
    return rc, need.value


def _planes(size, shift=0):
    """three poisoned planes of `size` bytes, `shift` bytes off a 4-byte boundary"""
    import torch
    return [torch.full((size + 4,), POISON, dtype=torch.uint8, device="cuda:0")[shift:shift + size] for _ in range(3)]


def _same_rows(got, want, total):
    for name, g, w in zip(("q_row", "a_row", "t_row"), got, want):
        g = g.cpu().numpy()
        bad = np.flatnonzero(g[:total] != w)
        assert bad.size == 0, f"{name}: first differing byte {bad[:1]} of {total}"
        assert (g[total:] == POISON).all(), name                  # nothing at or beyond d_row_off[n] is written


def _render_and_compare(al, a, want, only, shifts=(0, 1, 2, 3)):
    """the rows of arrays `a` into poisoned planes at every shift, against `want`; the inputs unchanged"""
    import torch
    ins = _inputs(a)
    before = [t.clone() for t in ins]
    n, total = len(a["status"]), len(want[0])
    for shift in shifts:
        planes = _planes(total + 61, shift)
        assert all(p.data_ptr() % 4 == shift for p in planes)
        off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
        out = al.alignment_text_tensors_packed(*ins[:7], q_rc=ins[7], only_aligned=bool(only), out=(*planes, off))
        assert all(x is y for x, y in zip(out, (*planes, off)))
        assert np.array_equal(off.cpu().numpy().view(np.uint64), want[3])
        _same_rows(planes, want, total)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))     # the inputs are only read
    return ins


@pytest.mark.parametrize("n", [1, 3, 4, 5, SCAN_BLOCK_PAIRS + 1])
@pytest.mark.parametrize("only", [0, 1])
@pytest.mark.parametrize("flags", FLAGS)
def test_synthetic_records(al, flags, only, n):
    picked, *want = _synthetic(n)
    want = want[only]
    total = len(want[0])
    assert total > 0
    a = P.arrays(picked, P.flags_of(flags, n), seed=100 + n)
    ins = _render_and_compare(al, a, want, only)
    # out=None: one sizing call, then exactly the rows; q_rc=None is the array of zeros
    q_row, a_row, t_row, o3 = al.alignment_text_tensors_packed(*ins[:7], q_rc=None if flags == "none" else ins[7], only_aligned=bool(only))
    assert q_row.numel() == a_row.numel() == t_row.numel() == total
    _same_rows((q_row, a_row, t_row), want, total)
    assert np.array_equal(o3.cpu().numpy().view(np.uint64), want[3])


def test_device_rows_equal_the_host_renderers(al):
    import wfa_amd
    n = 40
    picked, _, _ = _synthetic(n)
    a = P.arrays(picked, P.flags_of("alt", n))
    z = np.zeros(n, np.uint32)
    qbegin, qend, tbegin, tend = a["win"]
    br = wfa_amd.BatchResult(a["status"], z, tbegin, tend, qbegin, qend, z, z, z, z, a["ops_off"], a["ops_len"], a["ops"])
    ins = _inputs(a)
    for only in (False, True):
        host = wfa_amd.alignment_text_packed(br, *a["pk"], only_aligned=only, n_threads=3)
        dev = al.alignment_text_tensors_packed(*ins[:7], q_rc=ins[7], only_aligned=only)
        for h, d in zip(host, dev):
            assert np.array_equal(h.view(np.uint8), d.cpu().numpy().view(np.uint8))


SEAM_LENGTHS = list(range(1, 34)) + [47, 48, 49, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def test_word_seams_on_both_strands(al):
    """single-M pairs of every length 1 .. 33 and around 48, 64, 256 and 1 024, each forward and flagged: every len % 16 of the
    flagged funnel shift, every seam of the groups of four and of the sweeps of 256 columns"""
    rng = np.random.default_rng(23)
    cases, flags = [], []
    for n in SEAM_LENGTHS:
        for flag in (0, 1):
            cases.append((P.OK, [P.op("M", n)], P.acgt(rng, n), P.acgt(rng, n), 1, n, 1, n))
            flags.append(flag)
    a = P.arrays(cases, flags, seed=31)
    for only in (0, 1):
        _render_and_compare(al, a, A.expected(cases, only), only)


def test_trimmed_windows_at_every_residue(al):
    """QBEGIN - 1 at every residue 0 .. 15 with QEND short of the length, TBEGIN - 1 at another residue, both strands: a flagged
    window counts from the far end of the words"""
    rng = np.random.default_rng(29)
    ops = [P.op("I", 1), P.op("M", 20), P.op("X", 1), P.op("D", 2), P.op("M", 14), P.op("H", 3)]   # trimmed: 37 query and 35 target bases
    cases, flags = [], []
    for r in range(16):
        for extra in (0, 16, 32):      # the window in the first, second and third word
            tr = (5 * r + 3) % 16
            for flag in (0, 1):
                q, t = P.acgt(rng, r + extra + 37 + 5), P.acgt(rng, tr + 35 + 3)
                cases.append((P.OK, ops, q, t, r + extra + 1, r + extra + 37, tr + 1, tr + 35))
                flags.append(flag)
    assert {(c[4] - 1) % 16 for c in cases} == set(range(16)) and all(c[5] < len(c[2]) for c in cases)
    _render_and_compare(al, P.arrays(cases, flags, seed=37), A.expected(cases, 1), 1)


@pytest.mark.parametrize("n_ops", [65, 129, 200])
def test_groups_that_cross_op_boundaries(al, n_ops):
    """ops of counts 1, 2 and 3 -- no group of four columns lies inside one op -- and of counts 1 .. 6, over two, three and four
    rounds, both strands, both modes"""
    rng = np.random.default_rng(41 + n_ops)
    cases = []
    for top in (3, 6):
        made = A.make([P.op("MXIDH"[int(rng.integers(0, 5))], int(rng.integers(1, top + 1))) for _ in range(n_ops)], rng, slack=n_ops % 2)
        cases += [made, made]
    cases = P.with_acgt(cases, seed=n_ops)
    cases[1], cases[3] = cases[0], cases[2]            # each case twice, forward and flagged
    a = P.arrays(cases, [0, 1, 0, 1], seed=43)
    for only in (0, 1):
        _render_and_compare(al, a, A.expected(cases, only), only)


def test_sequences_that_share_words(al):
    """one query offset under two lengths and both flag values in one batch, and the query and the target of a pair on the same
    words: a flagged prefix is the reverse complement of THAT prefix"""
    rng = np.random.default_rng(47)
    s, u = P.acgt(rng, 100), P.acgt(rng, 61)
    words = np.concatenate([P.pack_seq(s), P.pack_seq(u)])
    u_at = P.packed_words(100)
    M = lambda n: [P.op("M", n)]
    # (case, q_woff, t_woff, flag); a case's query bytes are the strand the rows show
    layout = [((P.OK, M(100), s, s, 1, 100, 1, 100), 0, 0, 0),                                        # query and target: the same words
              ((P.OK, M(100), P.revcomp(s), s, 1, 100, 1, 100), 0, 0, 1),                             # ... and the query flagged
              ((P.OK, [P.op("M", 30), P.op("X", 7)], P.revcomp(s[:37]), s, 1, 37, 1, 37), 0, 0, 1),    # the same offset, 37 bases, flagged
              ((P.OK, [P.op("M", 30), P.op("X", 7)], s[:37], u, 1, 37, 1, 37), 0, u_at, 0),            # ... and forward
              ((P.OK, M(61), P.revcomp(u), u, 1, 61, 1, 61), u_at, u_at, 1),
              ((P.OK, [P.op("D", 3), P.op("M", 58)], u, s[:70], 4, 61, 1, 58), u_at, 0, 0)]            # a target that is a prefix
    cases = [x[0] for x in layout]
    pk = (words, np.array([x[1] for x in layout], np.uint64), np.array([len(c[2]) for c in cases], np.uint32),
          np.array([x[2] for x in layout], np.uint64), np.array([len(c[3]) for c in cases], np.uint32),
          np.array([x[3] for x in layout], np.uint8))
    a = _manual(cases, pk)
    for only in (0, 1):
        _render_and_compare(al, a, A.expected(cases, only), only, shifts=(0, 3))


@pytest.mark.parametrize("only", [0, 1])
def test_tail_bits_and_pad_words_do_not_count(al, only):
    n = 40
    picked, *want = _synthetic(n)
    fl = P.flags_of("alt", n)
    clean = P.arrays(picked, fl)
    for seed in (5, 6):
        junk = P.arrays(picked, fl, junk_tails=seed)
        assert not np.array_equal(junk["pk"][0], clean["pk"][0])
        _render_and_compare(al, junk, want[only], only, shifts=(0, 1))


def test_capacity_errors_and_sizing_call(al):
    import torch
    from wfa_amd import _lib
    n = 5
    picked, want, _ = _synthetic(n)
    ins = _inputs(P.arrays(picked, P.flags_of("alt", n)))
    total = len(want[0])
    planes = _planes(total + 64)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    rc, need = _raw(al, ins, 0, planes, total - 1, off)
    assert rc == _lib.ERR_OOM and need == total
    assert all((p.cpu().numpy() == POISON).all() for p in planes)                  # the planes untouched
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[3])              # d_row_off filled
    rc, need = _raw(al, ins, 0, planes, total, off)                                # exactly the total: fits
    assert rc == 0 and need == total
    _same_rows(planes, want, total)
    off.fill_(-1)
    rc, need = _raw(al, ins, 0, [None] * 3, 0, off)                                # the sizing call
    assert rc == _lib.ERR_OOM and need == total and np.array_equal(off.cpu().numpy().view(np.uint64), want[3])
    # no pairs: d_row_off[0] = 0 and nothing else
    off.fill_(-1)
    planes = _planes(64)
    rc, need = _raw(al, [ins[0][:0]] + ins[1:], 0, planes, 64, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0] + [-1] * n
    assert all((p.cpu().numpy() == POISON).all() for p in planes)


# (only_aligned, what is wrong, the same thing at the bound): changes to altext_pk_cases.PAIR -- 7 query bases, 9 target bases,
# trimmed 4M over query bases [1, 5) and target bases [2, 6)
CHECKS = [
    (0, dict(q_len=6), dict(q_len=7)),                      # the ops consume one query base more than there is
    (0, dict(t_len=8), dict(t_len=9)),                      # ... one target base
    (1, dict(qend=4), dict(qend=5)),                        # ... than the trimmed window holds
    (1, dict(tbegin=4), dict(tbegin=3)),
    (1, dict(qbegin=0), dict(qbegin=1)),                    # QBEGIN = 0
    (1, dict(tbegin=0, tend=3), dict(tbegin=1, tend=4)),
    (1, dict(qend=8), dict(qbegin=4, qend=7)),              # QEND = q_len + 1
    (1, dict(tend=10), dict(tbegin=6, tend=9)),
    (1, dict(qbegin=6, qend=4), dict(qbegin=2, qend=5)),    # QBEGIN - 1 > QEND
]


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("only,wrong,right", CHECKS)
def test_checks_of_the_length_kernel(al, only, wrong, right, flag):
    import torch
    from wfa_amd import _lib
    planes = _planes(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    rc, _need = _raw(al, _inputs(P.one(flag, **wrong)), only, planes, 256, off)
    assert rc == _lib.ERR_BAD_ARG
    assert all((p.cpu().numpy() == POISON).all() for p in planes)
    rc, need = _raw(al, _inputs(P.one(flag, **right)), only, planes, 256, off)
    assert rc == 0 and need == [11, 4][only]


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("only", [0, 1])
def test_words_or_ops_outside_their_buffers(al, only, flag):
    import torch
    from wfa_amd import _lib
    a = P.one(flag)
    words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
    ins = _inputs(a)
    planes = _planes(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    n_words = len(words)           # (the later sequence of the pair ends exactly there)
    ops_end = int(a["ops_off"][0] + a["ops_len"][0])
    for kw in (dict(n_words=n_words - 1), dict(ops_cap=ops_end - 1), dict(n_words=0)):
        rc, _need = _raw(al, ins, only, planes, 256, off, **kw)
        assert rc == _lib.ERR_BAD_ARG, kw
        assert all((p.cpu().numpy() == POISON).all() for p in planes)
    last = "q_woff" if q_woff[0] > t_woff[0] else "t_woff"
    at_bound = int((q_woff if last == "q_woff" else t_woff)[0])
    for v in (at_bound + 1, n_words, 1 << 63, (1 << 64) - 1):
        rc, _need = _raw(al, _inputs(P.one(flag, **{last: v})), only, planes, 256, off)
        assert rc == _lib.ERR_BAD_ARG, v
        assert all((p.cpu().numpy() == POISON).all() for p in planes)
    # the same offsets on a pair that is not OK are never looked at: nothing renders, nothing is refused
    b = P.one(flag, **{last: 1 << 63})
    b["status"][0] = K.NO_MEMORY
    rc, need = _raw(al, _inputs(b), only, planes, 256, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0, 0, 0]
    assert all((p.cpu().numpy() == POISON).all() for p in planes)
    rc, need = _raw(al, ins, only, planes, 256, off, n_words=n_words, ops_cap=ops_end)   # both end exactly at their bounds
    assert rc == 0 and need == [11, 4][only]
    got = [p.cpu().numpy() for p in planes]
    assert [g[:need].tobytes() for g in got] == list(A.rows_of(P.PAIR, only)) and all((g[need:] == POISON).all() for g in got)


def test_offsets_of_pairs_that_render_nothing_are_not_looked_at(al):
    """a pair without a column, and trimmed a pair without an M op, one word beyond n_words"""
    import torch
    from wfa_amd import _lib
    cases = [P.PAIR, P.NOT_OK, P.NO_COLUMN, (P.OK, [], b"", b"", 0, 0, 0, 0), (P.OK, [P.op("X", 2), P.op("I", 1)], b"AC", b"GTA", 1, 2, 1, 3)]
    a = P.arrays(cases, [1, 0, 1, 0, 1], seed=2)
    words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
    q_woff[2] = t_woff[2] = len(words)
    q_len[2] = t_len[2] = 1000
    _render_and_compare(al, a, A.expected(cases, 0), 0, shifts=(0,))
    q_woff[4] = len(words) - 1
    _render_and_compare(al, a, A.expected(cases, 1), 1, shifts=(0,))
    planes = _planes(64)
    off = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    rc, _need = _raw(al, _inputs(a), 0, planes, 64, off)       # untrimmed the X and I render: refused
    assert rc == _lib.ERR_BAD_ARG and all((p.cpu().numpy() == POISON).all() for p in planes)


def test_caller_owned_stream(al):
    import torch
    n = SCAN_BLOCK_PAIRS + 1
    picked, _, want = _synthetic(n)
    ins = _inputs(P.arrays(picked, P.flags_of("alt", n), seed=100 + n))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        q_row, a_row, t_row, off = al.alignment_text_tensors_packed(*ins[:7], q_rc=ins[7], only_aligned=True, stream=s)
    _same_rows((q_row, a_row, t_row), want, len(want[0]))
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[3])


def _mutated(rng, t, rate):
    out = bytearray()
    for b in t:
        x = rng.random()
        if x < rate / 3:
            continue                                              # a deletion
        if x < 2 * rate / 3:
            out.append(int(rng.choice(list(b"ACGT"))))            # an insertion
        out.append(int(rng.choice([c for c in b"ACGT" if c != b])) if 2 * rate / 3 <= x < rate else b)
    return bytes(out) or b"A"


@functools.lru_cache(maxsize=None)
def _batch(glob):
    """about 200 pairs of lengths 1 .. 300 and four of 1 kbp at 5 % error, every second one flagged; semi-global the targets
    overhang on both sides.  (strand queries, stored queries, targets, flags): a flagged query is stored reverse-complemented"""
    rng = np.random.default_rng(61 + glob)
    lengths = [int(x) for x in rng.integers(1, 301, 196)] + [1, 2, 16, 17, 1000, 1000, 1003, 990]
    ts = [P.acgt(rng, n) for n in lengths]
    qs = [_mutated(rng, t, 0.05) for t in ts]
    if not glob:
        ts = [P.acgt(rng, int(rng.integers(1, 60))) + t + P.acgt(rng, int(rng.integers(1, 60))) for t in ts]
    flags = [i & 1 for i in range(len(qs))]
    return qs, [P.revcomp(q) if f else q for q, f in zip(qs, flags)], ts, flags


def _rows(q_row, a_row, t_row, off):
    planes, o = [p.cpu().numpy().tobytes() for p in (q_row, a_row, t_row)], off.cpu().numpy()
    return [tuple(p[int(o[i]):int(o[i + 1])] for p in planes) for i in range(len(o) - 1)]


def _blob_to_device(arrays, pad=64):
    blob, q_off, q_len, t_off, t_len = arrays
    return (_dev(np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(pad, np.uint8)])), _dev(np.asarray(q_off, np.uint64)),
            _dev(np.asarray(q_len, np.uint32)), _dev(np.asarray(t_off, np.uint64)), _dev(np.asarray(t_len, np.uint32)))


@pytest.mark.parametrize("only", [False, True])
@pytest.mark.parametrize("glob", [True, False])
def test_end_to_end_behind_pack_and_align(built, glob, only):
    """pack_tensors -> align_tensors_packed(q_rc) -> alignment_text_tensors_packed, against alignment_text_tensors over a byte blob
    with the flagged queries reverse-complemented on the host and against the oracle's AlignmentText on those bytes.  Untrimmed
    with wf-adaptive off, where the ops consume exactly the sequences; trimmed with wf-adaptive (10, 50, 1)."""
    import wfa_amd
    qs, stored, ts, flags = _batch(glob)
    a = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=glob), device=0)
    try:
        if only:
            assert a.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*ADAPT)) is None
        d_stored = _blob_to_device(wfa_amd.make_blob(stored, ts))
        packed, q_woff, t_woff = a.pack_tensors(*d_stored)
        q_rc = _dev(np.array(flags, np.uint8))
        rec, ops = a.align_tensors_packed(packed, q_woff, d_stored[2], t_woff, d_stored[4], q_rc=q_rc)
        got = _rows(*a.alignment_text_tensors_packed(rec, ops, packed, q_woff, d_stored[2], t_woff, d_stored[4], q_rc=q_rc, only_aligned=only))
        # the byte entry on the same records and ops, over the bytes of the strand they speak of
        strand = wfa_amd.make_blob(qs, ts)
        d_strand = _blob_to_device(strand)
        assert got == _rows(*a.alignment_text_tensors(rec, ops, *d_strand, only_aligned=only))
    finally:
        a.close()
    w = O.align_batch(O.make_params(global_alignment=glob, adaptive=ADAPT if only else None), *strand, n_threads=8)
    assert (w.status == 0).all() and np.array_equal(rec.cpu().numpy()[:, 0], w.status)
    cases = [(0, [int(x) for x in w.pair_ops(i)], qs[i], ts[i], int(w.qbegin[i]), int(w.qend[i]), int(w.tbegin[i]), int(w.tend[i]))
             for i in range(len(qs))]
    assert got == [A.rows_of(c, only) for c in cases]
    assert sum(len(g[0]) for g in got) > 20000 and any(f and len(g[0]) > 900 for f, g in zip(flags, got))
