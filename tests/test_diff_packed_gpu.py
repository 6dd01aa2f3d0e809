"""GPU: the difference string rendered on the device from 2-bit packed words, both strands (include/wfa_hip.h:
wfahip_diff_text_packed_device; Aligner.diff_tensors_packed).  The kernels on the synthetic records and ops of tests/diff_cases.py over
ACGT sequences packed by tests/altext_pk_cases.py -- a flagged query stored as its reverse complement -- against the Python
restatement and the host entry, byte for byte, at every shift of the text off a 4-byte boundary, with everything behind the text
still poisoned and the inputs unchanged: the seams of the rounds, of the lane-per-op bound and of the scan blocks, ops of 70 001
columns, a match run of ten digits, trimmed windows at every residue of a word, sequences that share words, random tail bits and pad
words; the capacity and validation errors, each next to the same record at the bound; a caller-owned stream; and end to end behind
pack_tensors and align_tensors_packed, against the byte entry on the reverse-complemented bytes, the host entry over the oracle's
results, and the round trip target + string -> query.  No test hands the write kernel anything the length kernel has not accepted."""
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
import diff_cases as D  # noqa: E402
import diff_device as V  # noqa: E402

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
FLAGS = ["none", "all", "alt"]


@pytest.fixture(scope="module")
def al(built):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=True), device=0)
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def _cases():
    return P.with_acgt(D.cases())


def _manual(cases, pk, seed=9):
    """arrays for cases whose words the test lays out itself"""
    status, ops_off, ops_len, ops = K.lay_out([c[:2] for c in cases], seed=seed)
    return dict(status=status, ops_off=ops_off, ops_len=ops_len, ops=ops, win=A.windows(cases), pk=pk)


@pytest.mark.parametrize("n", [1, 3, 4, 5, V.SCAN_BLOCK_PAIRS + 1])
@pytest.mark.parametrize("only", [0, 1])
@pytest.mark.parametrize("flags", FLAGS)
def test_synthetic_records(al, flags, only, n):
    picked = V.pick(_cases(), n)
    want = D.expected(picked, only)   # (it does not depend on the flags: a case's query bytes are the strand its record speaks of)
    total = len(want[0])
    assert total > 0
    ins = V.render_and_compare(al, P.arrays(picked, P.flags_of(flags, n), seed=100 + n), picked, only)
    # out=None: one sizing call, then exactly the text; q_rc=None is the array of zeros
    text, off = al.diff_tensors_packed(*ins[:7], q_rc=None if flags == "none" else ins[7], only_aligned=bool(only))
    assert text.numel() == total
    V.same_text(text, want[0], total)
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])


@pytest.mark.parametrize("n_ops", [64, 65, 129, 200])
def test_round_seams(al, n_ops):
    cases = [c for c in _cases() if len(c[1] or []) == n_ops]
    assert cases
    cases = cases + cases                         # each case forward and flagged
    flags = [0] * (len(cases) // 2) + [1] * (len(cases) // 2)
    for only in (0, 1):
        V.render_and_compare(al, P.arrays(cases, flags, seed=n_ops), cases, only, shifts=(0, 3))


def test_lane_bound_seams_and_long_ops(al):
    """diff_cases.extra_cases over ACGT, each case forward and flagged: gaps of 15, 16 and 17 letters, X runs of 5 and 6 columns and
    across every residue of a group, one op of 70 001 columns of each kind"""
    cases = P.with_acgt(D.extra_cases() + [c for c in A.cases() if A.consumed(c[1] or [])[0] >= 70000], seed=3)
    cases = cases + cases
    flags = [0] * (len(cases) // 2) + [1] * (len(cases) // 2)
    for only in (0, 1):
        V.render_and_compare(al, P.arrays(cases, flags, seed=5), cases, only)


def test_ten_digit_match_run(al):
    """an M op of 1 000 000 007 columns: ten digits and not a word read for it; query and target are the same zero words, and the
    flagged query's first bases are the complement of the words' last"""
    import torch
    n = D.ten_digit_case(b"A", b"A")[1]
    win = [np.array([v, v], np.int32) for v in (3, n - 3, 3, n - 3)]
    ops = D.ten_digit_case(b"A", b"A")[0]
    rec = V.dev(A.records(np.zeros(2, np.int32), np.zeros(2, np.uint64), np.array([3, 3], np.uint32), win))
    words = torch.zeros(P.packed_words(n), dtype=torch.int32, device="cuda:0")
    off0, len2 = V.dev(np.zeros(2, np.uint64)), V.dev(np.array([n, n], np.uint32))
    q_rc = V.dev(np.array([0, 1], np.uint8))
    for only in (False, True):
        want = [b":%d" % D.TEN_DIGITS] * 2 if only else [D.ten_digit_case(b"A", b"A")[2], D.ten_digit_case(b"A", b"T")[2]]
        text, off = al.diff_tensors_packed(rec, V.dev(np.array(ops, np.uint64)), words, off0, len2, off0, len2, q_rc=q_rc, only_aligned=only)
        assert text.cpu().numpy().tobytes() == b"".join(want) and off.cpu().numpy().tolist() == [0, len(want[0]), len(want[0]) + len(want[1])]


def test_trimmed_windows_at_every_residue(al):
    """QBEGIN - 1 at every residue 0 .. 15 of the first three words with QEND short of the length, TBEGIN - 1 at another residue,
    both strands: a flagged window counts from the far end of the words.  The ops hold a gap the wave sweeps on each side."""
    rng = np.random.default_rng(29)
    ops = [P.op("I", 1), P.op("M", 20), P.op("X", 1), P.op("D", 18), P.op("M", 3), P.op("I", 17), P.op("X", 6), P.op("M", 14), P.op("H", 3)]
    _, wq, wt = A.consumed(ops[1:8])               # trimmed: 62 query and 61 target bases
    cases, flags = [], []
    for r in range(16):
        for extra in (0, 16, 32):                  # the window in the first, second and third word
            tr = (5 * r + 3) % 16
            for flag in (0, 1):
                q, t = P.acgt(rng, r + extra + wq + 5), P.acgt(rng, tr + wt + 3)
                cases.append((P.OK, ops, q, t, r + extra + 1, r + extra + wq, tr + 1, tr + wt))
                flags.append(flag)
    assert {(c[4] - 1) % 16 for c in cases} == set(range(16)) and all(c[5] < len(c[2]) for c in cases)
    V.render_and_compare(al, P.arrays(cases, flags, seed=37), cases, 1, shifts=(0, 1))


def test_sequences_that_share_words(al):
    """one query offset under two lengths and both flag values in one batch, and the query and the target of a pair on the same
    words: a flagged prefix is the reverse complement of THAT prefix"""
    rng = np.random.default_rng(47)
    s, u = P.acgt(rng, 100), P.acgt(rng, 61)
    words = np.concatenate([P.pack_seq(s), P.pack_seq(u)])
    u_at = P.packed_words(100)
    X = lambda n: [P.op("X", n)]
    # (case, q_woff, t_woff, flag); a case's query bytes are the strand the string spells
    layout = [((P.OK, X(100), s, s, 1, 100, 1, 100), 0, 0, 0),                                        # query and target: the same words
              ((P.OK, X(100), P.revcomp(s), s, 1, 100, 1, 100), 0, 0, 1),                             # ... and the query flagged
              ((P.OK, [P.op("M", 10), P.op("D", 20), P.op("X", 7)], P.revcomp(s[:37]), s, 1, 37, 1, 17), 0, 0, 1),   # the same offset, 37 bases, flagged
              ((P.OK, [P.op("M", 10), P.op("D", 20), P.op("X", 7)], s[:37], u, 1, 37, 1, 17), 0, u_at, 0),           # ... and forward
              ((P.OK, [P.op("I", 61), P.op("H", 61)], P.revcomp(u), u, 1, 61, 1, 61), u_at, u_at, 1),
              ((P.OK, [P.op("D", 3), P.op("M", 40), P.op("I", 18)], u[:43], s[:70], 4, 43, 1, 40), u_at, 0, 0)]   # prefixes of both
    cases = [x[0] for x in layout]
    pk = (words, np.array([x[1] for x in layout], np.uint64), np.array([len(c[2]) for c in cases], np.uint32),
          np.array([x[2] for x in layout], np.uint64), np.array([len(c[3]) for c in cases], np.uint32),
          np.array([x[3] for x in layout], np.uint8))
    a = _manual(cases, pk)
    for only in (0, 1):
        V.render_and_compare(al, a, cases, only, shifts=(0, 3))


@pytest.mark.parametrize("only", [0, 1])
def test_tail_bits_and_pad_words_do_not_count(al, only):
    n = 40
    picked = V.pick(_cases(), n)
    fl = P.flags_of("alt", n)
    clean = P.arrays(picked, fl)
    for seed in (5, 6):
        junk = P.arrays(picked, fl, junk_tails=seed)
        assert not np.array_equal(junk["pk"][0], clean["pk"][0])
        V.render_and_compare(al, junk, picked, only, shifts=(0, 1))


def test_capacity_errors_sizing_call_and_empty_batch(al):
    import torch
    from wfa_amd import _lib
    n = 5
    picked = V.pick(_cases(), n)
    want = D.expected(picked, 0)
    ins = V.inputs(P.arrays(picked, P.flags_of("alt", n)))
    total = len(want[0])
    text = V.text_buf(total + 64)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    rc, need = V.raw(al, ins, 0, text, total - 1, off)                             # one below the total
    assert rc == _lib.ERR_OOM and need == total
    assert V.untouched(text)                                                       # the text untouched
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])              # d_text_off filled
    rc, need = V.raw(al, ins, 0, text, total, off)                                 # exactly the total: fits
    assert rc == 0 and need == total
    V.same_text(text, want[0], total)
    off.fill_(-1)
    rc, need = V.raw(al, ins, 0, None, 0, off)                                     # the sizing call
    assert rc == _lib.ERR_OOM and need == total and np.array_equal(off.cpu().numpy().view(np.uint64), want[1])
    # no pairs: d_text_off[0] = 0 and nothing else
    off.fill_(-1)
    text = V.text_buf(64)
    rc, need = V.raw(al, [ins[0][:0]] + ins[1:], 0, text, 64, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0] + [-1] * n
    assert V.untouched(text)


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
SIZES = [15, 2]   # the bytes of PAIR's string: +g-tt:4*gc+a-ca, and trimmed :4


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("only,wrong,right", CHECKS)
def test_checks_of_the_length_kernel(al, only, wrong, right, flag):
    import torch
    from wfa_amd import _lib
    text = V.text_buf(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    rc, _need = V.raw(al, V.inputs(P.one(flag, **wrong)), only, text, 256, off)
    assert rc == _lib.ERR_BAD_ARG and V.untouched(text)
    rc, need = V.raw(al, V.inputs(P.one(flag, **right)), only, text, 256, off)
    assert rc == 0 and need == SIZES[only]


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("only", [0, 1])
def test_words_or_ops_outside_their_buffers(al, only, flag):
    import torch
    from wfa_amd import _lib
    a = P.one(flag)
    words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
    ins = V.inputs(a)
    text = V.text_buf(256)
    off = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    n_words = len(words)           # (the later sequence of the pair ends exactly there)
    ops_end = int(a["ops_off"][0] + a["ops_len"][0])
    for kw in (dict(size=n_words - 1), dict(ops_cap=ops_end - 1), dict(size=0)):
        rc, _need = V.raw(al, ins, only, text, 256, off, **kw)
        assert rc == _lib.ERR_BAD_ARG and V.untouched(text), kw
    last = "q_woff" if q_woff[0] > t_woff[0] else "t_woff"
    at_bound = int((q_woff if last == "q_woff" else t_woff)[0])
    for v in (at_bound + 1, n_words, 1 << 63, (1 << 64) - 1):
        rc, _need = V.raw(al, V.inputs(P.one(flag, **{last: v})), only, text, 256, off)
        assert rc == _lib.ERR_BAD_ARG and V.untouched(text), v
    # the same offsets on a pair that is not OK are never looked at: nothing renders, nothing is refused
    b = P.one(flag, **{last: 1 << 63})
    b["status"][0] = K.NO_MEMORY
    rc, need = V.raw(al, V.inputs(b), only, text, 256, off)
    assert rc == 0 and need == 0 and off.cpu().numpy().tolist() == [0, 0, 0] and V.untouched(text)
    rc, need = V.raw(al, ins, only, text, 256, off, size=n_words, ops_cap=ops_end)   # both end exactly at their bounds
    assert rc == 0 and need == SIZES[only]
    got = text.cpu().numpy()
    assert got[:need].tobytes() == D.diff_of(P.PAIR, only) and (got[need:] == V.POISON).all()


def test_offsets_of_pairs_that_render_nothing_are_not_looked_at(al):
    """a pair without a byte, and trimmed a pair without an M op, one word beyond n_words"""
    import torch
    from wfa_amd import _lib
    cases = [P.PAIR, P.NOT_OK, P.NO_COLUMN, (P.OK, [], b"", b"", 0, 0, 0, 0), (P.OK, [P.op("X", 2), P.op("I", 1)], b"AC", b"GTA", 1, 2, 1, 3)]
    a = P.arrays(cases, [1, 0, 1, 0, 1], seed=2)
    words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
    q_woff[2] = t_woff[2] = len(words)
    q_len[2] = t_len[2] = 1000
    V.render_and_compare(al, a, cases, 0, shifts=(0,))
    q_woff[4] = len(words) - 1
    ins = V.render_and_compare(al, a, cases, 1, shifts=(0, 2))
    off = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    text = V.text_buf(64)
    rc, _need = V.raw(al, ins, 0, text, 64, off)               # untrimmed the X and I render: refused
    assert rc == _lib.ERR_BAD_ARG and V.untouched(text)


def test_caller_owned_stream(al):
    import torch
    n = V.SCAN_BLOCK_PAIRS + 1
    picked = V.pick(_cases(), n)
    want = D.expected(picked, 1)
    ins = V.inputs(P.arrays(picked, P.flags_of("alt", n), seed=100 + n))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        text, off = al.diff_tensors_packed(*ins[:7], q_rc=ins[7], only_aligned=True, stream=s)
    V.same_text(text, want[0], len(want[0]))
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])


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
    """204 pairs: lengths 1 .. 300 and four of 1 kbp at 5 % error, every second one flagged; semi-global the targets overhang on
    both sides.  (strand queries, stored queries, targets, flags): a flagged query is stored reverse-complemented"""
    rng = np.random.default_rng(71 + glob)
    lengths = [int(x) for x in rng.integers(1, 301, 196)] + [1, 2, 16, 17, 1000, 1000, 1003, 990]
    ts = [P.acgt(rng, n) for n in lengths]
    qs = [_mutated(rng, t, 0.05) for t in ts]
    if not glob:
        ts = [P.acgt(rng, int(rng.integers(1, 60))) + t + P.acgt(rng, int(rng.integers(1, 60))) for t in ts]
    flags = [i & 1 for i in range(len(qs))]
    return qs, [P.revcomp(q) if f else q for q, f in zip(qs, flags)], ts, flags


def _strings(text, off):
    t, o = text.cpu().numpy().tobytes() if hasattr(text, "cpu") else bytes(text), off.cpu().numpy() if hasattr(off, "cpu") else off
    return [t[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)]


def _blob_to_device(arrays, pad=64):
    blob, q_off, q_len, t_off, t_len = arrays
    return (V.dev(np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(pad, np.uint8)])), V.dev(np.asarray(q_off, np.uint64)),
            V.dev(np.asarray(q_len, np.uint32)), V.dev(np.asarray(t_off, np.uint64)), V.dev(np.asarray(t_len, np.uint32)))


@pytest.mark.parametrize("only", [False, True])
@pytest.mark.parametrize("glob", [True, False])
def test_end_to_end_behind_pack_and_align(built, glob, only):
    """pack_tensors -> align_tensors_packed(q_rc) -> diff_tensors_packed, against diff_tensors over a byte blob with the flagged
    queries reverse-complemented on the host, against the host entry over the oracle's results on those bytes, and round: the
    target's window and the string give the query's window back.  Untrimmed with wf-adaptive off, where the ops consume exactly
    the sequences; trimmed with wf-adaptive (10, 50, 1)."""
    import wfa_amd
    qs, stored, ts, flags = _batch(glob)
    assert len(qs) == 204
    a = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=glob), device=0)
    try:
        if only:
            assert a.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*ADAPT)) is None
        d_stored = _blob_to_device(wfa_amd.make_blob(stored, ts))
        packed, q_woff, t_woff = a.pack_tensors(*d_stored)
        q_rc = V.dev(np.array(flags, np.uint8))
        rec, ops = a.align_tensors_packed(packed, q_woff, d_stored[2], t_woff, d_stored[4], q_rc=q_rc)
        got = _strings(*a.diff_tensors_packed(rec, ops, packed, q_woff, d_stored[2], t_woff, d_stored[4], q_rc=q_rc, only_aligned=only))
        # the byte entry on the same records and ops, over the bytes of the strand they speak of
        strand = wfa_amd.make_blob(qs, ts)
        assert got == _strings(*a.diff_tensors(rec, ops, *_blob_to_device(strand), only_aligned=only))
    finally:
        a.close()
    prm = dict(global_alignment=glob, adaptive=ADAPT if only else None)
    w = O.align_batch(O.make_params(**prm), *strand, n_threads=8)
    assert (w.status == 0).all() and np.array_equal(rec.cpu().numpy()[:, 0], w.status)
    br = wfa_amd.BatchResult(w.status, w.score, w.tbegin, w.tend, w.qbegin, w.qend, w.align_len, w.matches, w.gaps, w.gap_regions, w.ops_off,
                             w.ops_len, w.ops)
    assert got == _strings(*wfa_amd.diff_text(br, *strand, only_aligned=only))
    cases = [(0, [int(x) for x in w.pair_ops(i)], qs[i], ts[i], int(w.qbegin[i]), int(w.qend[i]), int(w.tbegin[i]), int(w.tend[i]))
             for i in range(len(qs))]
    assert got == [D.diff_of(c, only) for c in cases]
    chk, _, _ = wfa_amd.check_alignments(br, *strand, options=wfa_amd.Options(GlobalAlignment=glob))
    n_round = 0
    for i, c in enumerate(cases):
        if chk[i, 0] & wfa_amd.CHK_M_DIFFERS or not got[i]:
            continue
        q, t = (c[2][c[4] - 1:c[5]], c[3][c[6] - 1:c[7]]) if only else (c[2], c[3])
        assert D.apply_diff(t, got[i]) == q, i
        n_round += 1
    assert n_round >= 195 and sum(len(g) for g in got) > 4000 and any(f and len(g) > 150 for f, g in zip(flags, got))
