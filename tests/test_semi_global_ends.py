"""CPU: the batches of tests/semi_global_ends.py decide what tests/test_semi_global_ends_gpu.py claims to test -- proved from the
oracle alone, never from a kernel.  These are conditions on the inputs, not measurements.

Every pair of every setting the GPU tests run (a batch, one of three penalty sets, wf-adaptive off for ends_free() and 10/50/1
for ends_adapt(); all semi-global) goes through the oracle and is classified by
  * Ak = m - n, the diagonal the forward pass watches (wfa.go:235-239);
  * K = tend - qend, the diagonal of the alignment's last match run: where the backtrace started;
  * s_final = Result.n_scores: the score at which the forward pass stopped.  oracle/wfa_oracle.c sets it to the loop variable
    of wfa.go:228-251 when M[s][Ak] has reached the target's end, before backtraceStartPosistion lowers the score to that of
    the start cell -- so score < s_final says that the scan over the lower scores found something.
A batch on which K == Ak and score == s_final for nearly every pair (what wfa_amd.generate_pairs gives) cannot tell a right
end-cell rule from "Ak at the last score"; the counts below say that these batches can."""
import concurrent.futures
import functools

import numpy as np
import pytest

from oracle import oracle as O
from semi_global_ends import TC_STRIPE, axis, ends_adapt, ends_free

PENS = [(4, 6, 2), (2, 4, 2), (6, 4, 2)]
ADAPT = (10, 50, 1)
BATCHES = {"free": (ends_free, None), "adapt": (ends_adapt, ADAPT)}


def _seqs(data, i):
    blob, q_off, q_len, t_off, t_len = data
    return (blob[int(q_off[i]):int(q_off[i]) + int(q_len[i])].tobytes(), blob[int(t_off[i]):int(t_off[i]) + int(t_len[i])].tobytes())


@functools.lru_cache(maxsize=None)
def classify(name, pen):
    """[(n, m, Ak, K, score, s_final, qend, tend, status)] of a batch under one penalty set: every pair through O.Aligner
    (align_batch does not return n_scores), eight threads with an aligner each"""
    build, ad = BATCHES[name]
    data, kinds = build()

    def run(idx):
        al = O.Aligner(O.make_params(*pen, global_alignment=False, adaptive=ad))
        out = []
        for i in idx:
            q, t = _seqs(data, i)
            r = al.align(q, t)
            out.append((i, (len(q), len(t), len(t) - len(q), r.tend - r.qend, r.score, r.n_scores, r.qend, r.tend, r.status)))
        al.close()
        return out
    # longest rows first, dealt round-robin: the eight threads end together
    order = sorted(range(len(kinds)), key=lambda i: -(int(data[2][i]) + int(data[4][i])))
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        rows = dict(kv for part in ex.map(run, [order[j::8] for j in range(8)]) for kv in part)
    return tuple(rows[i] for i in range(len(kinds)))


@pytest.mark.parametrize("name", ["free", "adapt"])
def test_batch_layout(name):
    build, _ = BATCHES[name]
    data, kinds = build()
    blob, q_off, q_len, t_off, t_len = data
    assert build()[0] is data and not any(a.flags.writeable for a in data)  # built once, read-only
    assert len(kinds) == len(q_len) == len(t_len) and 90 <= len(kinds) <= 115
    assert not (q_off % 16).any() and not (t_off % 16).any()  # make_blob's layout
    assert q_len.min() >= 1 and t_len.min() >= 1
    for i in range(len(kinds)):
        q, t = _seqs(data, i)
        assert set(q) <= set(b"ACGT") and set(t) <= set(b"ACGT"), (i, kinds[i])
        if kinds[i].startswith("identical"):
            assert q == t
    n, m = q_len.astype(int), t_len.astype(int)
    assert min(n.min(), m.min()) == 120 and (n[[k == "identical" for k in kinds]] == 120).any()
    if name == "free":
        assert 6000 <= max(n.max(), m.max()) <= 6200 and 8900 <= (n + m).max() <= 9100
        assert sum(k.startswith("unrelated") for k in kinds) == 4
        # Ak on, and one diagonal either side of, the edge between two stripes of a team of three (team_slack = 1024)
        for b in (0, 1):
            for d in (-1, 0, 1, 2):
                i = [j for j, k in enumerate(kinds) if k.startswith(f"edge b={b} d={d}")]
                assert len(i) == 1
                KB, S = axis(int(n[i[0]]), int(m[i[0]]), 3, 1024)
                assert int(m[i[0]] - n[i[0]]) == KB + (b + 1) * S - 1 + d and S < TC_STRIPE and n[i[0]] + m[i[0]] - 1 > TC_STRIPE - 2
                assert (n[i[0]] > m[i[0]]) == (b == 0)
    else:
        assert np.abs(m - n).max() <= 12
        longer = np.maximum(n, m)
        short = int(((longer >= 1000) & (longer <= 1300)).sum())
        long_ = int(((longer >= 2060) & (longer <= 2300)).sum())
        assert short >= 35 and long_ >= 35 and short + long_ >= len(kinds) - 12  # (the rest: the 120-base pair and the small cores)
    for k in set(x.split("/")[0] for x in kinds if x.startswith(("contained", "overhang"))):  # both ways round
        assert k in kinds and k + "/q" in kinds, k
    for prefix in ("far", "edge", "repeat", "small") if name == "free" else ("repeat", "small"):
        assert any(x.startswith(prefix) and x.endswith("/q") for x in kinds) and any(x.startswith(prefix) and not x.endswith("/q") for x in kinds)


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("name", ["free", "adapt"])
def test_batches_decide_the_end_cell(name, pen):
    rows = classify(name, pen)
    kinds = BATCHES[name][0]()[1]
    n, m, Ak, K, score, s_final, qend, tend, status = (np.array(c) for c in zip(*rows))
    assert not status.any(), [kinds[i] for i in np.nonzero(status)[0]]
    counts = {
        "K < Ak": int((K < Ak).sum()), "K > Ak": int((K > Ak).sum()), "K == Ak": int((K == Ak).sum()),
        "score < s_final": int((score < s_final).sum()),
        "ends on the query's last base, tend < m": int(((qend == n) & (tend < m)).sum()),
        "ends on the target's last base, qend < n": int(((tend == m) & (qend < n)).sum()),
        "n > m": int((n > m).sum()), "n < m": int((n < m).sum()), "n == m": int((n == m).sum()),
        "K == Ak + 1": int((K == Ak + 1).sum()),  # where the upward scan's first cell decides, its override of the downward scan included
    }
    far = int((np.abs(K - Ak) >= TC_STRIPE).sum())
    two, three = int((n + m - 1 > TC_STRIPE).sum()), int((n + m - 1 > 2 * TC_STRIPE).sum())
    print(f"{name} pen={pen}: {counts}; |K - Ak| >= 4096: {far}; n + m - 1 > 4096: {two}, > 8192: {three}; "
          f"highest s_final {int(s_final.max())}, highest score {int(score.max())}")
    for what, c in counts.items():
        assert c >= 8, (what, c)
    if name == "free":
        assert far >= 4 and three >= 4
    else:
        assert two >= 20


def test_stripe_edge_pairs_end_far_from_the_edge():
    """the "edge" pairs put Ak on a stripe's edge and the hit far from it, on diagonal +-1: the downward scan starts in one
    workgroup's stripe, the upward one in the next, and the minima that decide come from a third place"""
    rows, kinds = classify("free", (4, 6, 2)), ends_free()[1]
    for i, k in enumerate(kinds):
        if k.startswith("edge"):
            n, m, Ak, K, score, s_final = rows[i][:6]
            assert abs(K) == 1 and score < s_final and abs(K - Ak) > 1000, (k, rows[i])
