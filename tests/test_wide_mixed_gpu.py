"""GPU: semi-global batches of mixed read lengths through the length-class routing of align_device (wfa_amd/csrc/wfa_host.hip,
wfa_wide_plan.hpp): every pair within wfa_wide_kernel's 2 047 bases runs on it, in a launch sized by its own class; longer pairs
take the ladder; packed input takes the kernel's packed prologue.  Every case against the oracle on every record field and every
CIGAR op, twice through one aligner over a poisoned arena.  Counts of handed-on pairs are asserted only where a docstring says so;
otherwise they are printed."""
import ctypes as C
import functools

import numpy as np
import pytest

from structured_pairs import SCORE_EDGE, SCORE_LONG, structured_batch
from test_bounded_gpu import _assert_bounded
from test_parity_gpu import FIELDS, _aligner, _oracle_params, _semi_global_cases, assert_batch_equal

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
N_LONG = 44  # pairs of the mixed batch beyond 2 047 bases: 40 of 2 048 .. 2 300, 4 of 9 000


def _generated(seed, n, length, err):
    import wfa_amd as w
    blob, q_off, q_len, t_off, t_len = w.generate_pairs(seed=seed, n_pairs=n, length=length, error_rate=err, n_threads=4)
    qs = [bytes(blob[int(q_off[i]):int(q_off[i]) + int(q_len[i])]) for i in range(n)]
    ts = [bytes(blob[int(t_off[i]):int(t_off[i]) + int(t_len[i])]) for i in range(n)]
    return qs, ts


@functools.lru_cache(maxsize=None)
def _mixed(with_long=True):
    """(data, is_long): about 600 semi-global shapes of 1 .. 700 bases, 80 pairs of 1 000 and 80 of 1 900 bases, 40 of 2 048 .. 2 300
    and 4 of 9 000, shuffled with a fixed seed.  with_long = False: the same batch without its 44 long pairs, in the same order."""
    import wfa_amd as w
    rng = np.random.default_rng(20260101)
    qs, ts = _semi_global_cases(rng, 600, 1, 700, flank=12)
    for seed, n, length, err in ((1, 80, 1000, 0.05), (2, 80, 1900, 0.05)):
        q, t = _generated(seed, n, length, err)
        qs += q
        ts += t
    long_from = len(qs)
    for seed, n, length, err in ((3, 10, 2048, 0.05), (4, 10, 2100, 0.05), (5, 10, 2200, 0.05), (6, 10, 2300, 0.05), (7, 4, 9000, 0.02)):
        q, t = _generated(seed, n, length, err)
        qs += q
        ts += t
    assert len(qs) - long_from == N_LONG
    order = np.random.default_rng(7).permutation(len(qs))
    is_long = np.array([max(len(qs[i]), len(ts[i])) > 2047 for i in order])
    assert int(is_long.sum()) == N_LONG and all((i >= long_from) == l for i, l in zip(order, is_long))
    if not with_long:
        order = order[~is_long]
    data = w.make_blob([qs[i] for i in order], [ts[i] for i in order])
    for a in data:
        a.setflags(write=False)
    return data, is_long


@functools.lru_cache(maxsize=None)
def _mixed_want(pen, ad):
    from oracle import oracle as O
    return O.align_batch(_oracle_params(False, ad, pen), *_mixed()[0], n_threads=8)


def _timing(al, what):
    tm = al.last_timing()
    print(f"{what}: kind {tm.main_kernel_kind}, wide {tm.n_packed_pairs}, others {tm.n_retried_pairs}, main launches {tm.n_main_launches}, "
          f"arena {tm.arena_bytes}")
    return tm


def _planned(ad, pen, **opts):
    al = _aligner(False, ad, pen)
    al.set_option("arena_poison", 1)
    al.set_option("wide_bin_min_pairs", 1)
    for k, v in opts.items():
        al.set_option(k, v)
    return al


def _assert_subset_equal(got, want, keep, what):
    """got: the records of the pairs `keep` of want's batch, in order"""
    idx = np.nonzero(keep)[0]
    assert np.array_equal(got.status, want.status[idx]), what
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)[idx]), (what, f)
    for j, i in enumerate(idx):
        assert np.array_equal(got.pair_ops(j), want.pair_ops(int(i))), (what, j)


@pytest.mark.parametrize("ad", [ADAPT, None])
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2)])
def test_mixed_batch(built, pen, ad):
    """The mixed batch starts on wfa_wide_kernel (kind 18; before there were classes: kind 0, one 9 000-base read moved the whole batch
    to the ladder).  Asserted: the kernel is offered every pair but the 44 long ones (n_retried_pairs >= 44, and wide + others = n);
    n_retried_pairs equals that of the same batch without its long pairs plus 44 -- a class's geometry does not depend on what else
    the batch holds; one class ("wide_classes" 0) and the ladder alone ("wide" 0) give the same records."""
    data, is_long = _mixed()
    want, n = _mixed_want(pen, ad), len(is_long)
    al = _planned(ad, pen)
    for rep in range(2):
        got = al.align_arrays(*data)
        tm = _timing(al, f"mixed pen={pen} ad={ad} rep={rep}")
        assert tm.main_kernel_kind == 18
        assert tm.n_retried_pairs >= N_LONG and tm.n_packed_pairs + tm.n_retried_pairs == n
        assert_batch_equal(got, want, f"mixed pen={pen} ad={ad} rep={rep}")
    others = tm.n_retried_pairs
    short = al.align_arrays(*_mixed(False)[0])
    ts = _timing(al, f"mixed without its long pairs pen={pen} ad={ad}")
    assert ts.main_kernel_kind == 18
    _assert_subset_equal(short, want, ~is_long, "mixed without its long pairs")
    assert others == ts.n_retried_pairs + N_LONG, (others, ts.n_retried_pairs)
    al.set_option("wide_classes", 0)
    got = al.align_arrays(*data)
    assert _timing(al, "mixed, one class").main_kernel_kind == 18
    assert_batch_equal(got, want, f"mixed, one class, pen={pen} ad={ad}")
    al.set_option("wide_classes", 1)
    al.set_option("wide", 0)
    got = al.align_arrays(*data)
    assert _timing(al, "mixed, ladder").main_kernel_kind != 18
    assert_batch_equal(got, want, f"mixed, ladder, pen={pen} ad={ad}")
    al.close()


def _join(*datas):
    """batches (blob, q_off, q_len, t_off, t_len) one after the other"""
    blobs, qo, ql, to, tl, base = [], [], [], [], [], 0
    for blob, q_off, q_len, t_off, t_len in datas:
        qo.append(q_off + np.uint64(base)), to.append(t_off + np.uint64(base)), ql.append(q_len), tl.append(t_len)
        blobs += [blob, np.zeros(-len(blob) % 16, dtype=np.uint8)]  # (every batch starts on a 16-byte boundary, as make_blob lays pairs out)
        base += len(blob) + (-len(blob) % 16)
    return tuple(np.concatenate(x) for x in (blobs, qo, ql, to, tl))


def _seams():
    import wfa_amd as w
    bounds = w.wide_class_bounds()
    return [(64, b - 7, b, 20260200 + b) for b in bounds[:-1]], bounds


@functools.lru_cache(maxsize=None)
def _seam_case(k, ad):
    """class seam k: 64 pairs of b - 7 .. b bases joined with 64 of b + 1 .. b + 8 (k = -1: 2 040 .. 2 047 with 2 048 .. 2 060) and
    the oracle's records"""
    from oracle import oracle as O
    seams, _ = _seams()
    if k < 0:
        lo, hi = SCORE_EDGE, SCORE_LONG
    else:
        n, l0, b, seed = seams[k]
        lo, hi = (n, l0, b, seed), (n, b + 1, b + 8, seed + 1)
    data = _join(structured_batch(*lo)[0], structured_batch(*hi)[0])
    return data, O.align_batch(_oracle_params(False, ad, (4, 6, 2)), *data, n_threads=8)


@pytest.mark.parametrize("ad", [ADAPT, None])
def test_class_seams(built, ad):
    """For every class bound b below 2 047: reads of b - 7 .. b bases with reads of b + 1 .. b + 8 -- a read of b + 1 bases staged into
    class b's rings would overrun them.  At 2 047 the longer half is the ladder's: kind 18 and n_retried_pairs >= 64, asserted."""
    seams, bounds = _seams()
    assert len(seams) == len(bounds) - 1
    al = _planned(ad, (4, 6, 2))
    for k in list(range(len(seams))) + [-1]:
        data, want = _seam_case(k, ad)
        longer = np.maximum(data[2], data[4])
        b = bounds[k]
        assert int((longer <= b).sum()) == 64 and int((longer > b).sum()) == 64 and longer.max() <= b + 13
        for rep in range(2):
            got = al.align_arrays(*data)
            tm = _timing(al, f"seam at {b} ad={ad} rep={rep}")
            assert tm.main_kernel_kind == 18
            if k < 0:
                assert tm.n_retried_pairs >= 64
            assert_batch_equal(got, want, f"seam at {b} ad={ad} rep={rep}")
    al.close()


def test_small_batch_rule(built):
    """Default options, 300 pairs of 300 bases with 8 of 2 300: below "wide_bin_min_pairs" no lists are built -- one class, and the
    kernel hands the eight back (kind 18 and n_retried_pairs >= 8, asserted)."""
    import wfa_amd as w
    from oracle import oracle as O
    q, t = _generated(11, 300, 300, 0.05)
    ql, tl = _generated(12, 8, 2300, 0.05)
    order = np.random.default_rng(3).permutation(308)
    qs, ts = q + ql, t + tl
    data = w.make_blob([qs[i] for i in order], [ts[i] for i in order])
    want = O.align_batch(_oracle_params(False, ADAPT), *data, n_threads=8)
    al = _aligner(False, ADAPT)
    al.set_option("arena_poison", 1)
    for rep in range(2):
        got = al.align_arrays(*data)
        tm = _timing(al, f"small batch rep={rep}")
        assert tm.main_kernel_kind == 18 and tm.n_retried_pairs >= 8
        assert_batch_equal(got, want, f"small batch rep={rep}")
    al.close()


def test_small_class_is_merged(built):
    """2 000 pairs of 150 bases with 10 of 1 000: the ten are fewer than a launch is worth -- they ride in a merged class or in the
    largest one.  Records equal; the counts are printed."""
    import wfa_amd as w
    from oracle import oracle as O
    q, t = _generated(21, 2000, 150, 0.05)
    ql, tl = _generated(22, 10, 1000, 0.05)
    order = np.random.default_rng(4).permutation(2010)
    qs, ts = q + ql, t + tl
    data = w.make_blob([qs[i] for i in order], [ts[i] for i in order])
    want = O.align_batch(_oracle_params(False, ADAPT), *data, n_threads=8)
    al = _planned(ADAPT, (4, 6, 2))
    for rep in range(2):
        got = al.align_arrays(*data)
        assert _timing(al, f"merged class rep={rep}").main_kernel_kind == 18
        assert_batch_equal(got, want, f"merged class rep={rep}")
    al.close()


@pytest.mark.parametrize("ad", [ADAPT, None])
def test_packed_input(built, ad):
    """The mixed batch through pack_pairs and align_arrays_packed: kind 18 (before: packed semi-global batches never took the kernel),
    and the same pairs on either side as the byte entry has -- both asserted.  Once more with "unpack_all" 1, the old route."""
    import wfa_amd as w
    pen = (4, 6, 2)
    data, _ = _mixed()
    want = _mixed_want(pen, ad)
    words, qw, tw = w.pack_pairs(*data)
    al = _planned(ad, pen)
    al.align_arrays(*data)
    tb = _timing(al, f"byte entry ad={ad}")
    for rep in range(2):
        got = al.align_arrays_packed(words, qw, data[2], tw, data[4])
        tp = _timing(al, f"packed entry ad={ad} rep={rep}")
        assert tp.main_kernel_kind == 18
        assert (tp.n_packed_pairs, tp.n_retried_pairs) == (tb.n_packed_pairs, tb.n_retried_pairs)
        assert_batch_equal(got, want, f"packed entry ad={ad} rep={rep}")
    al.set_option("unpack_all", 1)
    got = al.align_arrays_packed(words, qw, data[2], tw, data[4])
    _timing(al, f"packed entry, unpack_all ad={ad}")
    assert_batch_equal(got, want, f"packed entry, unpack_all, ad={ad}")
    al.close()


def test_device_entry(built):
    """The mixed batch through wfahip_align_batch_device: max_len = 0 and max_len = the true bound give the oracle's records; kind 18."""
    import torch
    from wfa_amd import _lib as L
    data, _ = _mixed()
    blob, q_off, q_len, t_off, t_len = data
    want, n = _mixed_want((4, 6, 2), ADAPT), len(q_len)
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(np.array(a)).to(dev) for a in (blob, q_off.view(np.int64), q_len.view(np.int32), t_off.view(np.int64), t_len.view(np.int32))]
    al = _planned(ADAPT, (4, 6, 2))
    prm = al._params()
    cap = int(want.ops_len.astype(np.int64).sum()) * 4 + 16 * n
    d_ops = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_rec = torch.zeros((n, L.REC_WORDS), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # (torch's fills are on its stream, the calls below on the context's own)
    for max_len in (0, int(max(q_len.max(), t_len.max()))):
        d_rec.zero_(), d_ops.zero_()
        torch.cuda.synchronize(dev)
        needed = C.c_uint64()
        L.check(L.lib().wfahip_align_batch_device(al._ctx, C.byref(prm), d[0].data_ptr(), blob.size, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                  d[4].data_ptr(), n, max_len, d_rec.data_ptr(), d_ops.data_ptr(), cap, C.byref(needed), None),
                "wfahip_align_batch_device")
        assert _timing(al, f"device entry max_len={max_len}").main_kernel_kind == 18
        rec, ops = d_rec.cpu().numpy().view(np.uint32), d_ops.cpu().numpy().view(np.uint64)
        assert np.array_equal(rec[:, L.REC_STATUS].view(np.int32), want.status)
        for f, w_ in (("score", L.REC_SCORE), ("tbegin", L.REC_TBEGIN), ("tend", L.REC_TEND), ("qbegin", L.REC_QBEGIN), ("qend", L.REC_QEND),
                      ("align_len", L.REC_ALIGN_LEN), ("matches", L.REC_MATCHES), ("gaps", L.REC_GAPS), ("gap_regions", L.REC_GAP_REGIONS),
                      ("ops_len", L.REC_OPS_LEN)):
            assert np.array_equal(rec[:, w_].astype(np.int64), getattr(want, f).astype(np.int64) & 0xFFFFFFFF), (max_len, f)
        off = rec[:, L.REC_OPS_OFF_LO].astype(np.uint64) | (rec[:, L.REC_OPS_OFF_HI].astype(np.uint64) << np.uint64(32))
        for i in range(n):
            assert np.array_equal(ops[int(off[i]):int(off[i]) + int(rec[i, L.REC_OPS_LEN])], want.pair_ops(i)), (max_len, i)
    al.close()


def test_bounded_entry(built):
    """align_arrays(.., max_score) on the mixed batch at the oracle's median score: status and score as test_bounded_gpu's rule states
    (semi-global pairs are filtered after their alignment: this shows that the classes' work lists reach the filter)."""
    data, _ = _mixed()
    want = _mixed_want((4, 6, 2), ADAPT)
    bound = int(np.median(want.score[want.status == 0]))
    al = _planned(ADAPT, (4, 6, 2))
    for rep in range(2):
        got = al.align_arrays(*data, max_score=bound)
        over = _assert_bounded(got, want, bound, f"bounded, mixed, rep={rep}")
        assert 0 < int(over.sum()) < len(want.status)
        assert _timing(al, f"bounded rep={rep}").main_kernel_kind == 18
    al.close()
