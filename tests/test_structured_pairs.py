"""CPU: the batches of tests/structured_pairs.py are what tests/test_structured_gpu.py assumes -- proved from the oracle alone
(its M wavefronts after every alignment), never from a kernel.  The GPU tests assert that no pair leaves wfa_lane_kernel (rows
of at most LN_W = 30 diagonals), the blocked kernels (windows of 32 or 64 diagonals that start centred on diagonal 0) or the
score kernels (SCORE_BAND = 248); that only means something if the inputs cannot make a correct kernel hand a pair on.

The same for tests/test_seams_gpu.py and the seam batches.  Their "wide" pairs (ten substitutions) are there to outgrow a narrow
pair's half row in wfa_duo_kernel, so what is proved of them comes from that kernel's constants (wfa_duo_cfg.hpp): no row spans
more than DUO_WIDE_MAX = 56 diagonals -- the kernel may not hand them on for their band -- and the widest spans more than
DUO_WIDEN_AT = 26 at 4/6/2 without wf-adaptive, where the GPU test wants pairs that widen and park, and at most 26 under every
other setting it runs, where it asserts that no pair is handed on."""
import numpy as np
import pytest

from oracle import oracle as O
from structured_pairs import BLK_SEAMS, DUO_SEAMS, LANE, LANE_EDGE, LONG_SEAM, RUNS, S200, SCORE_EDGE, SHORT, structured_batch

PENS = [(4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (2, 3, 1)]
ADAPT = (10, 50, 1)
# what the GPU tests run with an assertion that no pair is handed on: (batch, penalty sets); wf-adaptive 10/50/1 and off for each
CASES = [(SHORT, PENS), (LANE, PENS), (LANE_EDGE[239], PENS[:1]), (LANE_EDGE[240], PENS[:1]), (SCORE_EDGE, PENS[:3])]
# the seam batches, with the penalty sets tests/test_seams_gpu.py runs them under (all global; wf-adaptive 10/50/1 and off for each)
DUO_THREE = ((465, 480), (977, 992), (1985, 2000))  # the classes that run under 2/4/2 and 1/1/1 as well
CASES += ([(b, PENS[:3] if c in DUO_THREE else PENS[:1]) for c, b in DUO_SEAMS.items()] +
          [(b, PENS[:2] if c == (2001, 2016) else PENS[:1]) for c, b in BLK_SEAMS.items()] + [(LONG_SEAM, PENS[:1]), (S200, PENS[:1])])
MAX_ROW = 28   # diagonals in the widest row next() may compute (the lane kernel's rows hold 30)
MAX_DIAG = 14  # |k| of the outermost stored M cell
DUO_WIDE_MAX = 56  # wfa_duo_cfg.hpp: a wide pair whose band spans more diagonals is handed on
DUO_WIDEN_AT = 26  # ... and a narrow pair whose band spans more than this widens


def _seqs(data, i):
    blob, q_off, q_len, t_off, t_len = data
    return (blob[int(q_off[i]):int(q_off[i]) + int(q_len[i])].tobytes(), blob[int(t_off[i]):int(t_off[i]) + int(t_len[i])].tobytes())


@pytest.mark.parametrize("batch", [SHORT, LANE])
def test_batch_shape(batch):
    n_pairs, l_min, l_max, _ = batch
    data, kinds = structured_batch(*batch)
    blob, q_off, q_len, t_off, t_len = data
    assert len(kinds) == len(q_len) == len(t_len) == n_pairs
    assert {k: kinds.count(k) for k in ("ident", "runs", "end", "rep")} == {"ident": 40, "runs": 240, "end": 80, "rep": 40}
    longer = np.maximum(q_len, t_len)
    assert longer.max() <= l_max and longer.min() >= l_min
    assert int((longer == l_max).sum()) >= 10
    assert int(np.abs(q_len.astype(int) - t_len.astype(int)).max()) <= 4
    assert not (q_off % 16).any() and not (t_off % 16).any()  # (make_blob's layout)
    assert not any(a.flags.writeable for a in data)
    runs_seen = set()
    for i in range(n_pairs):
        q, t = _seqs(data, i)
        assert set(q) <= set(b"ACGT") and set(t) <= set(b"ACGT")
        if kinds[i] == "ident":
            assert q == t
        elif kinds[i] == "end":  # the shorter read ends on a run that the longer one continues
            s, l = (q, t) if len(q) < len(t) else (t, q)
            diff = [p for p in range(len(s)) if s[p] != l[p]]
            assert len(diff) == 1 and len(s) < len(l)
            runs_seen.add(len(s) - 1 - diff[0])
        elif kinds[i] == "rep":
            assert len(set(q) | set(t)) <= 4 and len(set(q[:9])) <= 3
    assert runs_seen == set(RUNS)
    assert structured_batch(*batch)[0] is data  # (built once)


def _check_rows(batch, pen, ad, wide=False):
    """every pair through the oracle; (widest row next() computes, outermost stored M diagonal, highest score) over the pairs that
    are not "wide" -- or, wide = True, over the wide ones alone, whose rows are held to DUO_WIDE_MAX and whose diagonals to nothing"""
    x, o, e = pen
    data, kinds = structured_batch(*batch)
    al = O.Aligner(O.make_params(*pen, global_alignment=True, adaptive=ad))
    widest, outer, top = 0, 0, 0
    max_row, max_diag = (DUO_WIDE_MAX, max(batch[2], 1)) if wide else (MAX_ROW, MAX_DIAG)
    for i in range(len(kinds)):
        if (kinds[i] == "wide") != wide:
            continue
        q, t = _seqs(data, i)
        n, m = len(q), len(t)
        assert max(n, m) <= batch[2] and set(q) <= set(b"ACGT") and set(t) <= set(b"ACGT")
        r = al.align(q, t)
        assert r.status == 0, (i, kinds[i])
        top = max(top, r.score)
        band = {}  # kept band of M[s], where it has one
        for s in range(r.score + 1):
            w = al.wavefront(0, s)
            if w is None or w[1] < w[0]:
                continue
            band[s] = (w[0], w[1])
            ks = [w[0] + j for j, raw in enumerate(w[2]) if raw]
            if ks:
                outer = max(outer, -min(ks), max(ks))
                assert -max_diag <= min(ks) and max(ks) <= max_diag, (i, kinds[i], s, min(ks), max(ks))
        # the range of next() at s (wfa.go:557-563): the sources' kept bands, one wider either side, clamped to the matrix.
        # One score past the last: a kernel may compute that range before it sees that the pair has ended.
        for s in range(1, r.score + 2):
            src = [band[s - d] for d in (x, o + e, e) if s - d in band]
            if not src:
                continue
            lo = max(min(b[0] for b in src) - 1, -(n - 1))
            hi = min(max(b[1] for b in src) + 1, m - 1)
            widest = max(widest, hi - lo + 1)
            assert hi - lo + 1 <= max_row, (i, kinds[i], s, lo, hi)
    al.close()
    return widest, outer, top


@pytest.mark.parametrize("ad", [ADAPT, None])
@pytest.mark.parametrize("batch,pen", [(b, p) for b, pens in CASES for p in pens])
def test_rows_stay_inside_the_kernels_windows(batch, pen, ad):
    widest, outer, top = _check_rows(batch, pen, ad)
    print(f"batch {batch} pen {pen} ad {ad}: widest next() range {widest}, outermost M diagonal {outer}, highest score {top}")
    assert 0 < widest <= MAX_ROW and outer <= MAX_DIAG
    if len(batch) > 4 and batch[4]:  # (wide_every)
        widest, outer, top = _check_rows(batch, pen, ad, wide=True)
        print(f"batch {batch} pen {pen} ad {ad}, wide pairs: widest next() range {widest}, outermost M diagonal {outer}, highest score {top}")
        assert 0 < widest <= DUO_WIDE_MAX
        if pen == (4, 6, 2) and ad is None:
            assert widest > DUO_WIDEN_AT  # pairs widen (and park) at this slot size
        else:
            assert widest <= DUO_WIDEN_AT  # nobody widens: the GPU test asserts that no pair is handed on


def test_seam_batch_shape():
    """one DUO_SEAMS batch: what is dealt with wide_every = 50, and that the class's last sequence word is filled"""
    batch = DUO_SEAMS[(465, 480)]
    n_pairs, l_min, l_max, _, wide_every = batch
    data, kinds = structured_batch(*batch)
    blob, q_off, q_len, t_off, t_len = data
    assert len(kinds) == len(q_len) == len(t_len) == n_pairs == 4099 and wide_every == 50
    assert [i for i in range(n_pairs) if kinds[i] == "wide"] == list(range(25, n_pairs, 50))
    # i mod 10: 410 x 0, 820 x 3 or 7, 410 x 5 of which 82 are wide, the other 2 459 runs
    assert {k: kinds.count(k) for k in set(kinds)} == {"ident": 410, "runs": 2459, "end": 820, "rep": 328, "wide": 82}
    longer = np.maximum(q_len, t_len)
    assert longer.max() == l_max and longer.min() >= l_min
    assert int((longer == l_max).sum()) >= 10
    for kind in ("ident", "runs", "end", "rep", "wide"):  # (the longer read of every tenth pair of each kind)
        assert int((longer[[k == kind for k in kinds]] == l_max).sum()) >= kinds.count(kind) // 10
    assert int(np.abs(q_len.astype(int) - t_len.astype(int)).max()) <= 4
    assert not (q_off % 16).any() and not (t_off % 16).any()
    assert set(np.unique(blob)) <= set(b"ACGT") | {0} and not any(a.flags.writeable for a in data)
    for i in range(25, n_pairs, 50):  # ten substitutions, no gap, evenly spread
        q, t = _seqs(data, i)
        diff = [p for p in range(len(q)) if q[p] != t[p]]
        assert len(q) == len(t) and len(diff) == 10 and min(np.diff(diff)) >= 16, (i, diff)
    # all the batches of the table: one class of seq_words = (max_len + 15) / 16 + 1 each, the longest read at its upper end
    for (lo, hi), b in DUO_SEAMS.items():
        assert b[:3] == (4099, lo, hi) and b[4] == 50 and hi - lo == 15 and hi % 16 == 0
    assert len({b[3] for b in list(DUO_SEAMS.values()) + list(BLK_SEAMS.values()) + [LONG_SEAM, S200]}) == len(DUO_SEAMS) + len(BLK_SEAMS) + 2
