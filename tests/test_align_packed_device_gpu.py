"""GPU: full alignment of device-resident 2-bit words (wfahip_align_batch_packed_device; Aligner.align_tensors_packed).  Every comparison
has three sides, as tests/test_align_rc_gpu.py's: the new entry on the caller's words and flags, in torch tensors; the host entry
align_arrays_packed_rc on the SAME words, offsets, lengths and flags; and the oracle on bytes whose flagged queries were
reverse-complemented on the host.  Every record field 0 .. 10 and the ops each record indexes must agree, and so must the route between
the first two sides (main_kernel_kind, n_packed_pairs, n_retried_pairs), each on a fresh aligner with the same options.  After every
call of the new entry its input tensors must hold what they held before."""
import ctypes as C

import numpy as np
import pytest

from test_parity_gpu import assert_batch_equal
from test_score_rc_gpu import ADAPT, MAX_SEQ_LEN, MODES, _lay, _mutate, _pair_of, _rand, _revcomp
from test_align_rc_gpu import _aligner, _alternate, _buffers, _generated, _oracle, _route

pytestmark = pytest.mark.gpu
PAIR_EMPTY, PAIR_TOO_LONG, PAIR_OVER_MAX = 1, 2, 8
SLACK = 4  # words behind the caller's words, which the entry may read


def _to_device(pk, flags):
    """the caller's arrays as the tensors align_tensors_packed takes, four words of slack behind the words; flags None = no tensor"""
    import torch
    packed, q_woff, q_len, t_woff, t_len = pk
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to("cuda:0")
    words = np.concatenate([np.asarray(packed, np.uint32), np.full(SLACK, 0xFFFFFFFF, np.uint32)])
    return [dev(words, np.int32), dev(np.asarray(q_woff, np.uint64), np.int64), dev(np.asarray(q_len, np.uint32), np.int32),
            dev(np.asarray(t_woff, np.uint64), np.int64), dev(np.asarray(t_len, np.uint32), np.int32),
            None if flags is None else dev(np.asarray(flags, np.uint8), np.uint8)]


def _as_batch(rec, ops):
    """(rec, ops) of the device entry as the host entries' struct of arrays: the fields of the pairs that are OK (the others' are 0, as
    the host entry reports them) and the ops each record indexes, gathered in pair order"""
    import wfa_amd
    r = rec.cpu().numpy().view(np.uint32)
    o = ops.cpu().numpy().view(np.uint64)
    st = r[:, 0].astype(np.int32)
    st = np.where(np.isin(st, (0, 1, 2, 8)), st, 4).astype(np.int32)  # (the host entries report every other status as NO_MEMORY)
    ok = st == 0
    f = lambda k, dt: np.ascontiguousarray(np.where(ok, r[:, k], np.uint32(0)), np.uint32).view(dt)
    ops_len = f(10, np.uint32)
    src = r[:, 11].astype(np.uint64) | (r[:, 12].astype(np.uint64) << np.uint64(32))
    for i in np.nonzero(ok)[0]:
        assert int(src[i]) + int(ops_len[i]) <= len(o), ("the record's ops leave the op buffer", i)
    dense = np.concatenate([o[int(src[i]):int(src[i]) + int(ops_len[i])] for i in np.nonzero(ok)[0]] + [np.zeros(0, np.uint64)])
    ops_off = np.concatenate([[0], np.cumsum(ops_len.astype(np.uint64))[:-1]]).astype(np.uint64)
    return wfa_amd.BatchResult(st, f(1, np.uint32), f(2, np.int32), f(3, np.int32), f(4, np.int32), f(5, np.int32), f(6, np.uint32),
                               f(7, np.uint32), f(8, np.uint32), f(9, np.uint32), ops_off, ops_len, dense)


def _call(al, tens, max_score=0, stream=None):
    before = [t.clone() if t is not None else None for t in tens]
    rec, ops = al.align_tensors_packed(*tens[:5], q_rc=tens[5], max_score=max_score, stream=stream)
    for a, b in zip(tens, before):
        assert a is None or bool((a == b).all()), "an input tensor was written"
    return _as_batch(rec, ops), rec, ops


def _three_dev(pk, flags, want, glob, adaptive, opts=None, what="", als=None, keep=False):
    """the new entry over pk and flags (device tensors); align_arrays_packed_rc over the same arrays on an aligner of its own; the oracle.
    Returns the new entry's result, its timing and -- keep, or als given -- the two aligners (closed here otherwise: the contexts of
    the long-pair cases hold arenas of many GB)"""
    al, ref = als or (None, None)
    try:
        al = al or _aligner(glob, adaptive, opts)
        got, _, _ = _call(al, _to_device(pk, flags))
        tn = al.last_timing()
        if not (keep or als):
            al.close()
            al = None
        ref = ref or _aligner(glob, adaptive, opts)
        host = ref.align_arrays_packed_rc(*pk, flags)
        th = ref.last_timing()
        print(what, "glob", glob, "adaptive", adaptive, "| device: kind, packed, retried", _route(tn), "| host entry:", _route(th))
        assert_batch_equal(got, want, what + ": against the oracle")
        assert_batch_equal(got, host, what + ": against the host entry on the same words")
        assert _route(tn) == _route(th), what
    except BaseException:
        keep = als = None
        raise
    finally:
        if not (keep or als):
            for a in (al, ref):
                if a is not None:
                    a.close()
    return got, tn, (al, ref)


def _three(logical, ts, flags, glob, adaptive, opts=None, what="", gap=0, fill=0, want=None):
    flags = np.asarray(flags, np.uint8)
    pk = _buffers(logical, ts, flags, gap, fill)[0]
    want = want if want is not None else _oracle(logical, ts, glob, adaptive)
    got, t, _ = _three_dev(pk, flags, want, glob, adaptive, opts, what)
    return got, t


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_word_boundaries(glob, adaptive):
    """every length 1 .. 40, 63 .. 65 and 224 .. 240 under both flags; ones in every tail bit, pad word and gap word"""
    rng = np.random.default_rng(81)
    pairs = [_pair_of(rng, ln, 0.06) for ln in list(range(1, 41)) + [63, 64, 65] + list(range(224, 241))]
    qs, ts = [p[0] for p in pairs] * 2, [p[1] for p in pairs] * 2
    flags = _alternate(len(qs))
    want = _oracle(qs, ts, glob, adaptive)
    a, ta = _three(qs, ts, flags, glob, adaptive, what="word boundaries, fill 0", want=want)
    b, tb = _three(qs, ts, flags, glob, adaptive, what="word boundaries, fill 1", gap=1, fill=0xFFFFFFFF, want=want)
    assert_batch_equal(a, b, "tail bits")
    assert _route(ta) == _route(tb)


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_first_pass_slots_1kbp(glob, adaptive):
    """520 x 1 000 bases at 5 % with duo = 2: wfa_prepack_words_kernel fills the first pass's slots from the caller's words"""
    qs, ts = _generated(82, 520, 1000, 0.05)
    _, t = _three(qs, ts, _alternate(len(qs)), glob, adaptive, {"duo": 2}, "1 kbp at 5 %", fill=0xFFFFFFFF)
    if glob:
        assert t.main_kernel_kind == 8 and (adaptive is None or (t.n_packed_pairs == len(qs) and t.n_retried_pairs == 0)), t


@pytest.mark.parametrize("glob,adaptive", MODES)
@pytest.mark.parametrize("lane_pack", [1, 0])
def test_lane_kernel_150_bases(glob, adaptive, lane_pack):
    qs, ts = _generated(83, 1500, 150, 0.02)
    _, t = _three(qs, ts, _alternate(len(qs)), glob, adaptive, {"lane": 2, "lane_pack": lane_pack}, f"150 bases, lane_pack {lane_pack}", fill=0xFFFFFFFF)
    if glob:
        assert t.main_kernel_kind == 10, t


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_wide_kernel_and_its_hand_on(glob, adaptive):
    """2 040 .. 2 060 bases among 90 reads of 200 .. 400: semi-global, wfa_wide_kernel's packed prologue and the ladder behind it"""
    rng = np.random.default_rng(84)
    pairs = [_pair_of(rng, ln, 0.03) for ln in range(2040, 2061)] + [_pair_of(rng, int(rng.integers(200, 400)), 0.04) for _ in range(90)]
    order = rng.permutation(len(pairs))
    qs, ts = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    _, t = _three(qs, ts, _alternate(len(qs)), glob, adaptive, {}, "2040..2060", fill=0xFFFFFFFF)
    if not glob:
        assert t.main_kernel_kind == 18 and t.n_retried_pairs >= 13, t


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_long_windows_and_their_rungs(glob, adaptive):
    """eight 12 000-base pairs among 300 of 1 000 bases: window passes from slots, rungs and the ladder from bytes (the options of
    tests/test_align_rc_gpu.py's case: slots per team, so that the count of retried pairs is the same from run to run)"""
    short = _generated(85, 300, 1000, 0.05)
    longp = _generated(86, 8, 12000, 0.05)
    qs, ts = short[0] + longp[0], short[1] + longp[1]
    flags = _alternate(len(qs))
    flags[300:] = [1, 0, 1, 1, 0, 1, 0, 1]
    opts = {"team_paged": 0, "duo": 0} if glob else {"team_paged": 0}
    _, t = _three(qs, ts, flags, glob, adaptive, opts, "long pairs among short ones", fill=0xFFFFFFFF)
    if glob:
        assert t.n_retried_pairs >= 8, t


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_team_kernels(glob, adaptive):
    qs, ts = _generated(87, 6, 700, 0.10)
    opts = {"packed": 0, "team_min_len": 1, "team_wgs": 3, "team_solo_max": 16}
    _three(qs, ts, [1, 0, 1, 1, 0, 1], glob, adaptive, opts, "team kernels", fill=0xFFFFFFFF)


@pytest.mark.parametrize("glob,adaptive", MODES)
@pytest.mark.parametrize("slots", [False, True])
def test_one_query_listed_six_times(glob, adaptive, slots):
    """one stored query: forward, flagged, flagged at a shorter length, forward at that length, flagged from a word offset inside it, and
    a flagged palindrome: the flagged listings share mirror bytes under three lengths"""
    rng = np.random.default_rng(88)
    L, S, W = 1000, 613, 7
    stored = _rand(rng, L)
    pal = b"ACGT" * 100
    logical = [stored, _revcomp(stored), _revcomp(stored[:S]), stored[:S], _revcomp(stored[16 * W:]), pal]
    listing = [(0, L, 0), (0, L, 1), (0, S, 1), (0, S, 0), (W, L - 16 * W, 1), (None, len(pal), 1)]
    filler = _generated(89, 260, 1000, 0.05)
    ts = [_mutate(rng, q, 0.05) for q in logical]
    seqs = [stored, pal] + ts + filler[0] + filler[1]  # every sequence ONCE
    packed, offs = _lay(seqs, gap=1, fill=0xFFFFFFFF)
    n6, nf = len(logical), len(filler[0])
    q_woff = np.array([int(offs[1]) if w is None else int(offs[0]) + w for w, _, _ in listing] + [int(o) for o in offs[2 + n6:2 + n6 + nf]], np.uint64)
    t_woff = np.array([int(o) for o in offs[2:2 + n6]] + [int(o) for o in offs[2 + n6 + nf:]], np.uint64)
    q_len = np.array([ln for _, ln, _ in listing] + [len(q) for q in filler[0]], np.uint32)
    t_len = np.array([len(t) for t in ts + filler[1]], np.uint32)
    flags = np.array([f for _, _, f in listing] + [0] * nf, np.uint8)
    all_q, all_t = logical + filler[0], ts + filler[1]
    opts = {"duo": 2} if slots else {"duo": 0, "prepack": 0}
    _, t, _ = _three_dev((packed, q_woff, q_len, t_woff, t_len), flags, _oracle(all_q, all_t, glob, adaptive), glob, adaptive, opts,
                         f"six listings, slots {slots}")
    if glob and slots:
        assert t.main_kernel_kind == 8, t


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_empty_and_too_long_pairs(glob, adaptive):
    """set flags on empty and too long pairs, their offsets far outside the buffer: never looked at"""
    rng = np.random.default_rng(90)
    qs = [_rand(rng, int(rng.integers(100, 400))) for _ in range(24)]
    ts = [_mutate(rng, q, 0.05) for q in qs]
    qs[2], ts[5] = b"", b""
    flags = (np.arange(24) % 2).astype(np.uint8)
    flags[[2, 5, 6]] = 1
    pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)[0]
    pk[2][6] = MAX_SEQ_LEN + 1  # too long
    pk[1][6], pk[1][2] = np.uint64(1 << 40), np.uint64((1 << 64) - 1)
    pk[3][2], pk[3][5] = np.uint64(1 << 41), np.uint64(1 << 63)
    qs_o, ts_o = list(qs), list(ts)
    qs_o[6] = b""
    want = _oracle(qs_o, ts_o, glob, adaptive)
    want.status[6] = PAIR_TOO_LONG
    got, _, _ = _three_dev(pk, flags, want, glob, adaptive, None, "empty and too long")
    assert got.status[2] == PAIR_EMPTY and got.status[5] == PAIR_EMPTY and got.status[6] == PAIR_TOO_LONG


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_stale_mirror_and_a_byte_call_behind_it(glob, adaptive):
    """a second, smaller call with other data on the same aligners: nothing of the first call's mirror may be read; then a byte-input
    align_tensors call on the aligner that has just run flagged packed calls: the packed state is gone, the result is the oracle's"""
    import torch
    import wfa_amd
    qs, ts = _generated(91, 300, 400, 0.10)
    flags = _alternate(len(qs))
    pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)[0]
    _, _, als = _three_dev(pk, flags, _oracle(qs, ts, glob, adaptive), glob, adaptive, {"learn": 0}, "first call", keep=True)
    try:
        qs2, ts2 = _generated(92, 120, 390, 0.10)
        flags2 = (np.arange(len(qs2)) % 3 != 0).astype(np.uint8)
        pk2 = _buffers(qs2, ts2, flags2)[0]
        _three_dev(pk2, flags2, _oracle(qs2, ts2, glob, adaptive), glob, adaptive, None, "second call", als=als)
        arrays = wfa_amd.make_blob(qs, ts)
        dts = (np.uint8, np.int64, np.int32, np.int64, np.int32)
        tens = [torch.from_numpy(np.ascontiguousarray(a).view(dt)).to("cuda:0") for a, dt in zip(arrays, dts)]
        rec, ops = als[0].align_tensors(*tens)
        assert_batch_equal(_as_batch(rec, ops), _oracle(qs, ts, glob, adaptive), "byte input behind a flagged packed call")
    finally:
        for a in als:
            a.close()


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_unpack_all(glob, adaptive):
    rng = np.random.default_rng(93)
    pairs = [_pair_of(rng, int(rng.integers(1, 700)), 0.05) for _ in range(200)] + [_pair_of(rng, 2050, 0.03)]
    qs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    _three(qs, ts, _alternate(len(qs)), glob, adaptive, {"unpack_all": 1}, "unpack_all", gap=1, fill=0xFFFFFFFF)


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_no_flags_is_the_call_without_flags(glob, adaptive):
    """q_rc=None and all-zero flags: the same records, ops and timing fields, and those of the host entry without flags"""
    qs, ts = _generated(94, 300, 500, 0.05)
    pk = _buffers(qs, ts, np.zeros(len(qs), np.uint8))[0]
    want = _oracle(qs, ts, glob, adaptive)
    fields = ("n_launches", "n_retried_pairs", "arena_bytes", "n_main_launches", "n_packed_pairs", "main_kernel_kind", "ops_written",
              "ladder_start_level")
    seen, recs = [], []
    for how in ("none", "zeros"):
        al = _aligner(glob, adaptive)
        got, rec, ops = _call(al, _to_device(pk, None if how == "none" else np.zeros(len(qs), np.uint8)))
        assert_batch_equal(got, want, how)
        t = al.last_timing()
        seen.append(tuple(getattr(t, f) for f in fields))
        recs.append((rec.cpu().numpy(), got))
        al.close()
    assert seen[0] == seen[1], seen
    assert np.array_equal(recs[0][0][:, :11], recs[1][0][:, :11])
    assert_batch_equal(recs[0][1], recs[1][1], "none against zeros")
    ref = _aligner(glob, adaptive)
    assert_batch_equal(recs[0][1], ref.align_arrays_packed(*pk), "against align_arrays_packed")
    assert _route(ref.last_timing()) == (seen[0][5], seen[0][4], seen[0][1])
    ref.close()


@pytest.mark.parametrize("glob", [True, False])
def test_bounded_against_the_byte_entry(glob):
    """max_score at the batch's median score: align_arrays(max_score=) on the bytes, flagged queries reverse-complemented on the host"""
    import wfa_amd
    qs, ts = _generated(95, 400, 600, 0.08)
    flags = _alternate(len(qs))
    pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)[0]
    full = _oracle(qs, ts, glob, ADAPT)
    bound = int(np.median(full.score[full.status == 0]))
    al, ref = _aligner(glob, ADAPT), _aligner(glob, ADAPT)
    try:
        got, rec, _ = _call(al, _to_device(pk, flags), max_score=bound)
        want = ref.align_arrays(*wfa_amd.make_blob(qs, ts), max_score=bound)
        over = want.status == PAIR_OVER_MAX
        assert over.sum() > 20 and (want.status == 0).sum() > 20
        assert_batch_equal(got, want, "bounded")
        r = rec.cpu().numpy()
        assert (r[over, 0] == PAIR_OVER_MAX).all() and not r[over, 1:11].any()
    finally:
        al.close(), ref.close()


def test_short_op_buffer_and_offsets_outside_the_words():
    """the raw entry: WFAHIP_ERR_OOM with ops_needed on a short op buffer, then success with that capacity; WFAHIP_ERR_BAD_ARG for
    woff + words > n_words and for an offset that would wrap, with d_rec and d_ops untouched"""
    import torch
    from wfa_amd import _lib
    qs, ts = _generated(96, 200, 300, 0.05)
    flags = _alternate(len(qs))
    pk = _buffers(qs, ts, flags, fill=0xFFFFFFFF)[0]
    want = _oracle(qs, ts, True, ADAPT)
    al = _aligner(True, ADAPT)
    f = _lib.lib().wfahip_align_batch_packed_device
    try:
        tens = _to_device(pk, flags)
        n, n_words = len(qs), tens[0].numel() - SLACK
        prm = al._params()

        def run(t, cap):
            rec = torch.full((n, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            ops = torch.full((max(cap, 1),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
            need = C.c_uint64(0)
            torch.cuda.synchronize()
            rc = f(al._ctx, C.byref(prm), t[0].data_ptr(), n_words, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                   t[5].data_ptr(), n, 0, 0, rec.data_ptr(), ops.data_ptr(), cap, C.byref(need), None)
            torch.cuda.synchronize()
            return rc, rec, ops, need.value
        rc, _, _, need = run(tens, 16)
        assert rc == _lib.ERR_OOM and need > 16
        rc, rec, ops, need2 = run(tens, need)
        assert rc == 0 and need2 <= need
        assert_batch_equal(_as_batch(rec, ops), want, "after the sizing call")
        lens = pk[2].astype(np.uint64)
        for which, idx, off in ((1, 7, np.uint64(n_words) - (lens[7] + 15) // 16), (3, 9, np.uint64(n_words)), (1, 0, np.uint64((1 << 64) - 1)),
                                (3, 4, np.uint64((1 << 64) - 2)), (1, 5, np.uint64(1 << 63))):
            bad = [a.copy() for a in pk]
            bad[which][idx] = off  # (the first: the sequence's words fit, its pad word does not)
            rc, rec, ops, _ = run(_to_device(bad, flags), need)
            assert rc == _lib.ERR_BAD_ARG, (which, idx, off)
            assert bool((rec == 0x5A5A5A5A).all()) and bool((ops == 0x5A5A5A5A5A5A5A5A).all()), "d_rec / d_ops were touched"
        rc, rec, ops, _ = run(tens, need)  # ... and the context is as good as before
        assert rc == 0
        assert_batch_equal(_as_batch(rec, ops), want, "after the refused calls")
    finally:
        al.close()


def test_chain_generate_pack_align_cigar():
    """generate_pairs_device -> pack_tensors -> align_tensors_packed(q_rc=) -> cigar_tensors: the text of the oracle's results on the
    same bytes with the flagged queries reverse-complemented on the host; no sequence byte leaves the device on the way"""
    import torch
    import wfa_amd
    al = _aligner(True, ADAPT)
    try:
        n = 600
        blob, q_off, q_len, t_off, t_len = wfa_amd.generate_pairs_device(al, seed=97, n_pairs=n, length=300, error_rate=0.05)
        packed, q_woff, t_woff = al.pack_tensors(blob, q_off, q_len, t_off, t_len)
        flags = _alternate(n)
        s = torch.cuda.Stream(device="cuda:0")
        rec, ops = al.align_tensors_packed(packed, q_woff, q_len, t_woff, t_len, q_rc=torch.from_numpy(flags).to("cuda:0"), stream=s)
        text, off = al.cigar_tensors(rec, ops, stream=s)
        hb = blob.cpu().numpy()
        seq = lambda o, k: [bytes(hb[int(a):int(a) + int(b)]) for a, b in zip(o.cpu().numpy(), k.cpu().numpy())]
        qs = [_revcomp(q) if f else q for q, f in zip(seq(q_off, q_len), flags)]
        want = _oracle(qs, seq(t_off, t_len), True, ADAPT)
        assert_batch_equal(_as_batch(rec, ops), want, "the chain's records")
        wt, wo = wfa_amd.cigar_text(want)
        assert np.array_equal(off.cpu().numpy().view(np.uint64), wo) and text.cpu().numpy().tobytes() == wt.tobytes()
        assert (want.status == 0).all() and len(wt) > n
    finally:
        al.close()
