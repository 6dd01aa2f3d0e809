"""CPU: the batches of tests/structured_pairs.py are what tests/test_structured_gpu.py assumes -- proved from the oracle alone
(its M wavefronts after every alignment), never from a kernel.  The GPU tests assert that no pair leaves wfa_lane_kernel (rows
of at most LN_W = 30 diagonals), the blocked kernels (windows of 32 or 64 diagonals that start centred on diagonal 0) or the
score kernels (SCORE_BAND = 248); that only means something if the inputs cannot make a correct kernel hand a pair on."""
import numpy as np
import pytest

from oracle import oracle as O
from structured_pairs import LANE, LANE_EDGE, RUNS, SCORE_EDGE, SHORT, structured_batch

PENS = [(4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (2, 3, 1)]
ADAPT = (10, 50, 1)
# what the GPU tests run with an assertion that no pair is handed on: (batch, penalty sets); wf-adaptive 10/50/1 and off for each
CASES = [(SHORT, PENS), (LANE, PENS), (LANE_EDGE[239], PENS[:1]), (LANE_EDGE[240], PENS[:1]), (SCORE_EDGE, PENS[:3])]
MAX_ROW = 28   # diagonals in the widest row next() may compute (the lane kernel's rows hold 30)
MAX_DIAG = 14  # |k| of the outermost stored M cell


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


def _check_rows(batch, pen, ad):
    """every pair through the oracle; (widest row next() computes, outermost stored M diagonal, highest score)"""
    x, o, e = pen
    data, kinds = structured_batch(*batch)
    al = O.Aligner(O.make_params(*pen, global_alignment=True, adaptive=ad))
    widest, outer, top = 0, 0, 0
    for i in range(len(kinds)):
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
                assert -MAX_DIAG <= min(ks) and max(ks) <= MAX_DIAG, (i, kinds[i], s, min(ks), max(ks))
        # the range of next() at s (wfa.go:557-563): the sources' kept bands, one wider either side, clamped to the matrix.
        # One score past the last: a kernel may compute that range before it sees that the pair has ended.
        for s in range(1, r.score + 2):
            src = [band[s - d] for d in (x, o + e, e) if s - d in band]
            if not src:
                continue
            lo = max(min(b[0] for b in src) - 1, -(n - 1))
            hi = min(max(b[1] for b in src) + 1, m - 1)
            widest = max(widest, hi - lo + 1)
            assert hi - lo + 1 <= MAX_ROW, (i, kinds[i], s, lo, hi)
    al.close()
    return widest, outer, top


@pytest.mark.parametrize("ad", [ADAPT, None])
@pytest.mark.parametrize("batch,pen", [(b, p) for b, pens in CASES for p in pens])
def test_rows_stay_inside_the_kernels_windows(batch, pen, ad):
    widest, outer, top = _check_rows(batch, pen, ad)
    print(f"batch {batch} pen {pen} ad {ad}: widest next() range {widest}, outermost M diagonal {outer}, highest score {top}")
    assert 0 < widest <= MAX_ROW and outer <= MAX_DIAG
