"""GPU: WF_EXTEND's continuation paths, the read ends and tied next() sources of the short-read, semi-global and score kernels,
on the batches of tests/structured_pairs.py (identical pairs, exact runs one base either side of every extension round, runs
that end on the shorter read's last base, repeats) against the CPU oracle.  Random ACGT rarely matches for more than 16 bases,
so the rest of the suite hardly reaches wfa_lane_kernel's second round and third sequence word, wfa_blk_kernel's path behind
its first window, wfa_wide_kernel's sv.lcp loop or the pad-word clamp of SeqView<0>::lcp.

The full-alignment tests compare every record field and every CIGAR op, twice through one aligner over a poisoned arena, and
pin the kernel (main_kernel_kind); the score tests compare status and score.  Where a test asserts n_retried_pairs == 0 -- the
kernel named did all the work, not the one behind it -- tests/test_structured_pairs.py proves on the CPU, from the oracle alone,
that the batch allows it: no row of next() spans more than 28 diagonals and no M cell lies further than 14 diagonals from the
main one, under these penalties, wf-adaptive on or off."""
import functools

import numpy as np
import pytest

from structured_pairs import LANE, LANE_EDGE, SCORE_EDGE, SCORE_LONG, SHORT, structured_batch
from test_parity_gpu import _aligner, _oracle_params, assert_batch_equal

pytestmark = pytest.mark.gpu
ADAPT = (10, 50, 1)
ADS = [ADAPT, None]
PENS = [(4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (2, 3, 1)]


@functools.lru_cache(maxsize=None)
def _want(batch, glob, pen, ad, ops=True):
    """the oracle's records of a batch: computed once, shared by the tests that run it"""
    from oracle import oracle as O
    return O.align_batch(_oracle_params(glob, ad, pen), *structured_batch(*batch)[0], n_threads=8, want_ops=ops)


def _full(batch, glob, pen, ad, opts, kind, none_handed_on, what, max_handed_on=None, packed=False):
    """twice through one aligner over a poisoned arena: kind, records, CIGARs; returns the aligner (still open).
    max_handed_on: a bound on n_retried_pairs where some pairs may leave; packed: through pack_pairs and align_arrays_packed"""
    data = structured_batch(*batch)[0]
    want = _want(batch, glob, pen, ad)
    assert not np.any(want.status)
    al = _aligner(glob, ad, pen)
    for k, v in opts.items():
        al.set_option(k, v)
    al.set_option("arena_poison", 1)
    if packed:
        import wfa_amd
        words, qw, tw = wfa_amd.pack_pairs(*data)
    for rep in range(2):
        got = al.align_arrays_packed(words, qw, data[2], tw, data[4]) if packed else al.align_arrays(*data)
        tm = al.last_timing()
        print(f"{what} pen={pen} ad={ad} rep={rep}: kind {tm.main_kernel_kind}, handed on {tm.n_retried_pairs}")
        if kind is not None:
            assert tm.main_kernel_kind == kind
        if none_handed_on:
            assert tm.n_retried_pairs == 0, f"{what}: pairs left the kernel, their records come from the one behind it"
        if max_handed_on is not None:
            assert tm.n_retried_pairs <= max_handed_on, f"{what}: more pairs left the kernel than could have had to"
        assert_batch_equal(got, want, f"{what} pen={pen} ad={ad} rep={rep}")
    return al


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", PENS)
def test_lane_kernel(built, pen, ad):
    """wfa_lane_kernel, a lane per pair: reads of 224 to 240 bases -- the third sequence word, rounds two and three of its
    extension, offsets of 240 and 241 in its byte rings.  Rows of at most 28 diagonals never meet its hi - lo + 1 > LN_W."""
    _full(LANE, True, pen, ad, {"lane": 2}, 10, True, "lane").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("length", [239, 240, 241])
def test_lane_kernel_length_limit(built, length, ad):
    """every pair's longer read at the kernel's limit of 240 bases, one under, and one over (which it does not take: parity only)"""
    take = length <= 240
    _full(LANE_EDGE[length], True, (4, 6, 2), ad, {"lane": 2}, 10 if take else None, take, f"lane L={length}").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", PENS[:3])
def test_blocked_kernel_16_lanes(built, pen, ad):
    """wfa_blk_kernel, 16 lanes and a 64-diagonal window per pair.  The window starts centred on diagonal 0 and moves only when
    a kept row touches its edge: cells within 14 diagonals of the main one never do, so no pair is handed on for its band."""
    _full(LANE, True, pen, ad, {"lane": 0, "blk_narrow": 0}, 3, True, "blk 16").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", PENS[:2])
def test_blocked_kernel_short_read_instance(built, pen, ad):
    """the 8-lane instance that batches of reads under 200 bases start on: 32-diagonal windows, eight pairs per wave, staged in
    groups.  Diagonals -14 .. 14 lie inside a window of 32 centred on diagonal 0 without touching its edge."""
    _full(SHORT, True, pen, ad, {"lane": 0}, 6, True, "blk 8, short reads").close()


@pytest.mark.parametrize("ad", ADS)
def test_blocked_kernel_8_lanes(built, ad):
    """the plain 8-lane instance (blk = 8) on the 224 .. 240 batch; what it hands on is printed, not asserted"""
    _full(LANE, True, (4, 6, 2), ad, {"blk": 8}, 4, False, "blk 8").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 3, 1)])
def test_generic_kernel(built, pen, ad):
    _full(LANE, True, pen, ad, {"packed": 0}, 0, False, "generic").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", PENS[:2])
def test_wide_kernel_semi_global(built, pen, ad):
    """wfa_wide_kernel, the default for semi-global reads: its sv.lcp loop behind the side-by-side first window, end cells on every
    diagonal of the last row and column.  Nothing asserted on n_retried_pairs: under wf-adaptive the repeats score about 146
    here, and the arena is not what this test is about."""
    what = "wide, semi-global"
    data, want = structured_batch(*LANE)[0], _want(LANE, False, pen, ad)
    al = _full(LANE, False, pen, ad, {}, 18, False, what)
    for opt in ("wide_waves", "wide_exact"):  # a wave per pair; every round on the exact per-cell path
        al.set_option(opt, 1)
        assert_batch_equal(al.align_arrays(*data), want, f"{what}, {opt} = 1, pen={pen} ad={ad}")
        al.set_option(opt, 0)
    if ad is not None:  # every pair runs to its end in the wide rings
        al.set_option("wide", 3)
        assert_batch_equal(al.align_arrays(*data), want, f"{what}, one phase, pen={pen} ad={ad}")
    al.close()


def _to_device(data):
    import torch
    blob, q_off, q_len, t_off, t_len = data
    host = (np.concatenate([blob, np.zeros(64, np.uint8)]), q_off.view(np.int64), q_len.view(np.int32), t_off.view(np.int64), t_len.view(np.int32))
    return tuple(torch.from_numpy(a.copy()).to("cuda:0") for a in host)


def _three_entries(al, batch, glob, pen, ad, kind, none_handed_on, what):
    """score_arrays, score_arrays_packed and score_tensors on one batch: status and score of the oracle, the kernel, pairs handed on"""
    import wfa_amd
    data = structured_batch(*batch)[0]
    want = _want(batch, glob, pen, ad, False)
    assert not np.any(want.status)
    packed, qw, tw = wfa_amd.pack_pairs(*data)
    dev = _to_device(data)
    for entry, call in (("bytes", lambda: al.score_arrays(*data)), ("packed", lambda: al.score_arrays_packed(packed, qw, data[2], tw, data[4])),
                        ("device", lambda: tuple(x.cpu().numpy() for x in al.score_tensors(*dev)))):
        st, sc = call()
        tm = al.last_timing()
        print(f"{what} {entry} glob={glob} pen={pen} ad={ad}: kind {tm.main_kernel_kind}, handed on {tm.n_retried_pairs}")
        assert tm.main_kernel_kind == kind, (what, entry)
        bad = np.nonzero((st != want.status) | (sc.view(np.uint32) != want.score))[0]
        assert len(bad) == 0, f"{what} {entry} glob={glob} pen={pen} ad={ad}: {len(bad)} pairs differ, first {bad[:5]}: {sc.view(np.uint32)[bad[:5]]} vs {want.score[bad[:5]]}"
        if none_handed_on:
            assert tm.n_retried_pairs == 0, (what, entry)


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", PENS[:3])
@pytest.mark.parametrize("glob", [True, False])
def test_score_entries(built, glob, pen, ad):
    """the score kernels (19 global, 20 semi-global) through the three score entries: the 224 .. 240 batch, and 64 pairs of
    2 040 to 2 047 bases -- an identical pair, end pairs and repeats up against SCORE_MAX_LEN and the 16-bit ring offsets, where
    SeqView<0>::lcp's clamp at the pad word is all that stops a run.  Global rows of 28 diagonals are far inside SCORE_BAND = 248."""
    al = _aligner(glob, ad, pen)
    kind = 19 if glob else 20
    _three_entries(al, LANE, glob, pen, ad, kind, glob, "score, 224..240")
    _three_entries(al, SCORE_EDGE, glob, pen, ad, kind, glob and ad is not None, "score, 2040..2047")
    al.close()


@pytest.mark.parametrize("ad", ADS)
def test_score_long_kernel(built, ad):
    """the same pairs just past SCORE_MAX_LEN, on wfa_score_long_kernel (score_long_min = 1: a batch of 64 is below its gate)"""
    al = _aligner(True, ad)
    al.set_option("score_long_min", 1)
    _three_entries(al, SCORE_LONG, True, (4, 6, 2), ad, 23, False, "score, 2048..2060")
    al.close()
