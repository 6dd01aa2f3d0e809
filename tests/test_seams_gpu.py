"""GPU: every read length at which the router's integer arithmetic changes the kernel or its layout, on the batches of
tests/structured_pairs.py against the CPU oracle.  wfa_host.hip computes seq_words = (max_len + 15) / 16 + 1 from a batch's
longest read; from it follow wfa_duo_kernel's slot (PW = 4 + 2 * ((seq_words + 1) & ~1) words, 256 / PW pairs per fetch, PW <= 256),
the blocked kernel's LDS (lds_d <= 20 KB), the sliding-window kernels' gate (max_len > long_min_len = 4 000) and
wfa_wide_kernel's (max_len <= WIDE_MAX_LEN = 2 047).  A capacity rule that is off by one in any of them corrupts a neighbour's
LDS or reads a word past a slot.  Every batch lies in one 16-base class (one seq_words) with reads of exactly l_max bases, and holds
what random reads never bring to a slot's last words: identical pairs, long exact runs, runs that end on a read's last base, repeats.

Every test compares every record field and every CIGAR op, twice through one aligner over a poisoned arena, and pins the kernel
(main_kernel_kind).  Where n_retried_pairs == 0 is asserted, tests/test_structured_pairs.py proves on the CPU, from the oracle
alone, that the batch allows it under these penalties and wf-adaptive settings; the other values are printed."""
import pytest

from structured_pairs import BLK_SEAMS, DUO_CLASSES, DUO_SEAMS, LONG_SEAM, S200, SCORE_EDGE, SCORE_LONG, structured_batch
from test_parity_gpu import assert_batch_equal
from test_structured_gpu import ADS, _full, _want

pytestmark = pytest.mark.gpu
DUO_THREE = ((465, 480), (977, 992), (1985, 2000))  # a class of 3, 1 and 1 pairs per fetch: all three penalty sets, and packed input


def _duo_opts(cls):
    """wfa_duo_kernel whatever the batch size; one wave per CU (256 waves for 4 099 pairs: every wave fetches, prefetches and
    refills its half rows several times -- without it the grid grows with the batch and no half row is ever refilled)"""
    opts = {"duo": 2, "packed_waves_per_cu": 1}
    if cls[1] <= 240:
        opts["duo_short"] = 2
    return opts


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("cls,pen", [(c, p) for c in DUO_CLASSES for p in ([(4, 6, 2), (2, 4, 2), (1, 1, 1)] if c in DUO_THREE else [(4, 6, 2)])])
def test_duo_fetch_classes(built, cls, pen, ad):
    """wfa_duo_kernel at both ends of every pairs-per-fetch class: 4 099 pairs (the queue ends on a partial fetch of every
    size), one pair in fifty with ten substitutions.

      longest read   seq_words   PW    pairs per fetch
       193 ..  208       14       32         8
       209 ..  224       15       36         7      (seq_words odd: the slot carries an unused word per sequence)
       225 ..  240       16       36         7
       241 ..  256       17       40         6
       257 ..  272       18       40         6
       273 ..  288       19       44         5
       321 ..  336       22       48         5
       337 ..  352       23       52         4
       449 ..  464       30       64         4
       465 ..  480       31       68         3
       609 ..  624       40       84         3
       625 ..  640       41       88         2
       961 ..  976       62      128         2
       977 ..  992       63      132         1
      1985 .. 2000      126      256         1      (the slot that one 16-byte load per lane exactly covers)

    At 4/6/2 without wf-adaptive the ten-substitution pairs widen and park (rows of 35 diagonals; DUO_WIDEN_AT = 26, DUO_WIDE_MAX
    = 56): one may be handed on only because its wave's four park records are full, so at most as many pairs leave as the batch
    has wide ones.  Under every other setting no row spans more than 26 diagonals, nobody widens, and no pair may leave."""
    batch = DUO_SEAMS[cls]
    widen = pen == (4, 6, 2) and ad is None
    n_wide = structured_batch(*batch)[1].count("wide")
    assert n_wide == 82
    _full(batch, True, pen, ad, _duo_opts(cls), 8, not widen, f"duo {cls}", max_handed_on=n_wide if widen else None).close()


@pytest.mark.parametrize("cls", DUO_THREE)
def test_duo_fetch_classes_packed_input(built, cls):
    """the same batches through pack_pairs and align_arrays_packed: wfa_prepack_words_kernel fills the slots -- the 256-word one
    among them -- from the uploaded words.  The kernel is the byte entry's."""
    batch, pen, ad = DUO_SEAMS[cls], (4, 6, 2), ADS[0]
    al = _full(batch, True, pen, ad, _duo_opts(cls), 8, True, f"duo {cls}, bytes")
    kind = al.last_timing().main_kernel_kind
    al.close()
    al = _full(batch, True, pen, ad, _duo_opts(cls), kind, True, f"duo {cls}, packed input", packed=True)
    assert al.last_timing().main_kernel_kind == kind == 8
    al.close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2)])
def test_duo_gate_at_2000_bases(built, pen, ad):
    """2 001 .. 2 016 bases: seq_words = 127, a slot of 260 words -- more than a fetch covers.  wfa_duo_kernel must not take the batch
    even when asked for (duo = 2): the 16-lane blocked kernel does, and keeps every pair (the window argument of
    test_structured_gpu.test_blocked_kernel_16_lanes)."""
    _full(BLK_SEAMS[(2001, 2016)], True, pen, ad, {"duo": 2}, 3, True, "duo gate, 2001..2016").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("case", ["3985..4000", "10193..10208", "10209..10224", "200"])
def test_blocked_kernel_at_its_length_limits(built, case, ad):
    """wfa_blk_kernel, 16 lanes: the longest reads it is the default for (long_min_len = 4 000); the longest it takes at all
    (long = 0; 10 208 bases: seq_words = 639, lds_d = 20 464 of 20 480 bytes) and the 16 bases past them, which it must refuse
    (parity only: those pairs land on the long-pair ladder); and 200 bases, one past the short-read instance's max_len < 200."""
    pen = (4, 6, 2)
    if case == "3985..4000":
        _full(BLK_SEAMS[(3985, 4000)], True, pen, ad, {}, 3, True, "blk 16, 3985..4000").close()
    elif case == "10193..10208":
        _full(BLK_SEAMS[(10193, 10208)], True, pen, ad, {"long": 0}, 3, True, "blk 16, 10193..10208").close()
    elif case == "10209..10224":
        al = _full(BLK_SEAMS[(10209, 10224)], True, pen, ad, {"long": 0}, None, False, "past blk 16, 10209..10224")
        assert al.last_timing().main_kernel_kind != 3
        al.close()
    else:
        _full(S200, True, pen, ad, {}, 3, True, "blk 16, 200").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("window_words", [64, 240])
@pytest.mark.parametrize("first", [0, 11, 12, 13, 14, 15])
def test_long_window_kernels_at_their_shortest_reads(built, first, window_words, ad):
    """the sliding-window kernels (kinds 11 .. 15) on reads only just long enough for them, 4 001 .. 4 016 bases: with the default
    window of 240 words (3 840 bases) a pair repositions once, a few bases before its reads end -- inside the last run of the "end"
    pairs and inside the identical pairs' only run; with 64 words, dozens of times.  first = 0: by batch size, a wave per pair."""
    opts = {"long_first": first, "long_window_words": window_words}
    _full(LONG_SEAM, True, (4, 6, 2), ad, opts, first or 15, False, f"long windows, first={first} words={window_words}").close()


@pytest.mark.parametrize("ad", ADS)
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2)])
def test_wide_kernel_at_2047_bases(built, pen, ad):
    """wfa_wide_kernel, semi-global full alignment, up against WIDE_MAX_LEN = 2 047 (16-bit ring offsets, 12-bit arena offsets):
    2 040 .. 2 047 bases are its, 2 048 .. 2 060 are not.  n_retried_pairs is printed only: under wf-adaptive the repeats score over a
    thousand here and may outgrow the arena."""
    what = "wide, semi-global, 2040..2047"
    data, want = structured_batch(*SCORE_EDGE)[0], _want(SCORE_EDGE, False, pen, ad)
    al = _full(SCORE_EDGE, False, pen, ad, {}, 18, False, what)
    for opt in ("wide_waves", "wide_exact"):  # a wave per pair; every round on the exact per-cell path
        al.set_option(opt, 1)
        assert_batch_equal(al.align_arrays(*data), want, f"{what}, {opt} = 1, pen={pen} ad={ad}")
        al.set_option(opt, 0)
    al.close()
    al = _full(SCORE_LONG, False, pen, ad, {}, None, False, "past wide, semi-global, 2048..2060")
    assert al.last_timing().main_kernel_kind != 18
    al.close()
