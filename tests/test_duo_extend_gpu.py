"""GPU: WF_EXTEND of wfa_duo_kernel (first 16-base window of a lane's four diagonals, then the continuation in 32-base rounds)
on inputs built so that extension is what can go wrong, against the CPU oracle: records and CIGARs of every pair.

The batch (about 2 000 pairs of 260 to 300 bases, the shortest reads the kernel takes; built once) holds
  * identical pairs: one run over the whole read;
  * exact-match runs of 15, 16, 17 / 31, 32, 33 / 47, 48, 49 / 64, 65 / 79, 80, 81 bases between mismatches -- one base either side
    of the end of the first window (16) and of the first, second (16 + 32) and third (16 + 64) round of the continuation --
    each started at text offsets = 0 and = 15 (mod 16), with the query on the same diagonal and one diagonal either side
    (the two sequences' windows then start at different bit positions of their words);
  * the same runs ending exactly at the end of the shorter sequence, n != m either way round: the window reads past the
    sequence's last word, and only the clamp by the bases that are left keeps padding from counting;
  * homopolymers and di-/trinucleotide repeats with a few substitutions and a length difference: every diagonal of a lane
    (and of its neighbours) runs long in the same step;
  * one pair in fifty with ten substitutions: its band outgrows a half row, so some lanes step as part of a 16-lane pair.
Every pair's score stays low enough for wfa_duo_kernel's window with wf-adaptive off as well (a band of s/2 - 2 diagonals either
side of the main one at score s: at most 23 diagonals for the bulk, 39 for the wide ones; a pair is handed on beyond 56), so
no pair may leave the kernel: n_retried_pairs == 0, or the test would be checking the retry kernel."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("score", "tbegin", "tend", "qbegin", "qend", "align_len", "matches", "gaps", "gap_regions", "ops_len")
RUNS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 79, 80, 81)
N_PAIRS = 2000
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _other(base):
    """a base that differs from `base` (A -> C -> G -> T -> A)"""
    return ACGT[(int(np.nonzero(ACGT == base)[0][0]) + 1) % 4]


def _subst(seq, pos):
    seq[pos] = _other(seq[pos])


def _runs_pair(rng, run, start_mod, shift, n_more):
    """t random; q = t with a substitution just before text offset P (P = start_mod mod 16), an exact run of `run` bases from P,
    a substitution after it, then n_more further runs from RUNS; shift = +1 / -1: one base of the first stretch dropped from
    q / added to q, so the runs lie one diagonal off the main one (and still start at text offset P)."""
    L = int(rng.integers(261, 300))
    t = ACGT[rng.integers(0, 4, L)]
    q = t.copy()
    P = 16 * int(rng.integers(1, 3)) + start_mod  # 16, 32 / 31, 47
    cuts, pos = [P - 1], P + run
    for _ in range(1 + n_more):
        if pos >= L - 1:
            break
        cuts.append(pos)
        pos += 1 + int(RUNS[rng.integers(0, len(RUNS))])
    for c in cuts:
        _subst(q, c)
    if shift > 0:
        q = np.delete(q, 5)
    elif shift < 0:
        q = np.insert(q, 5, _other(q[5]))
    return q, t


def _end_pair(rng, run, d, q_short):
    """the shorter sequence is a prefix of the longer one (d bases shorter), with a substitution `run` + 1 bases before its
    end: the last run ends exactly at the end of the shorter sequence"""
    L = int(rng.integers(264, 301))
    long_ = ACGT[rng.integers(0, 4, L)]
    short = long_[:L - d].copy()
    _subst(short, len(short) - run - 1)
    if rng.integers(0, 2):
        _subst(short, int(rng.integers(20, 100)))
    return (short, long_) if q_short else (long_, short)


def _repeat_pair(rng, unit, d, n_sub):
    """both sequences the same repeat, d bases apart in length, n_sub substitutions by a base the repeat does not contain"""
    u = np.frombuffer(unit, dtype=np.uint8)
    L = int(rng.integers(262, 297))
    t = np.tile(u, L // len(u) + 2)[:L].copy()
    q = np.tile(u, L // len(u) + 2)[:L + d].copy()
    foreign = ACGT[[b not in u for b in ACGT]][0]
    for p in rng.integers(10, L - 10, n_sub):
        q[p] = foreign
    return (q, t) if rng.integers(0, 2) else (t, q)


def _wide_pair(rng):
    """ten substitutions: score 40 at 4/6/2 -- a band of 35 diagonals without wf-adaptive, more than a half row holds"""
    L = int(rng.integers(280, 301))
    t = ACGT[rng.integers(0, 4, L)]
    q = t.copy()
    for p in np.linspace(12, L - 12, 10).astype(int) + rng.integers(-5, 6, 10):
        _subst(q, int(p))
    return q, t


@functools.lru_cache(maxsize=None)
def _batch():
    rng = np.random.default_rng(20240611)
    plan = [(r, a, s) for r in RUNS for a in (0, 15) for s in (0, 1, -1)]
    ends = [(r, d, qs) for r in RUNS for d in (1, 3) for qs in (True, False)]
    reps = [(u, d, ns) for u in (b"A", b"C", b"AC", b"GT", b"ACG") for d in (0, 1, 2, 4) for ns in (0, 2)]
    pairs = []
    for i in range(N_PAIRS):
        if i % 50 == 25:
            pairs.append(_wide_pair(rng))
        elif i % 10 == 0:
            L = int(rng.integers(260, 301))
            t = ACGT[rng.integers(0, 4, L)]
            pairs.append((t.copy(), t))
        elif i % 10 in (3, 7):
            pairs.append(_end_pair(rng, *ends[(i // 10 * 2 + (i % 10 == 7)) % len(ends)]))
        elif i % 10 == 5:
            pairs.append(_repeat_pair(rng, *reps[(i // 10) % len(reps)]))
        else:
            r, a, s = plan[(i * 7 + i // 10) % len(plan)]
            pairs.append(_runs_pair(rng, r, a, s, n_more=int(rng.integers(0, 4))))
    q_len = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
    t_len = np.array([len(t) for _, t in pairs], dtype=np.uint32)
    both = np.stack([q_len, t_len], axis=1).astype(np.uint64).ravel()
    offs = np.concatenate([[0], np.cumsum(both)[:-1]]).astype(np.uint64)
    blob = np.concatenate([np.concatenate(p) for p in pairs] + [np.zeros(16, dtype=np.uint8)])
    data = (blob, offs[0::2].copy(), q_len, offs[1::2].copy(), t_len)
    for a in data:
        a.setflags(write=False)
    return data


@pytest.mark.parametrize("ad", [(10, 50, 1), None])
@pytest.mark.parametrize("pen", [(4, 6, 2), (2, 4, 2)])
def test_duo_extend_matches_oracle(built, pen, ad):
    import wfa_amd as w
    from oracle import oracle as O
    data = _batch()
    n = len(data[2])
    al = w.New(w.Penalties(*pen), w.Options(GlobalAlignment=True), device=0)
    if ad is not None:
        assert al.AdaptiveReduction(w.AdaptiveReductionOption(*ad)) is None
    al.set_option("duo", 2)
    got = al.align_arrays(*data)
    tm = al.last_timing()
    al.close()
    assert tm.main_kernel_kind == 8
    assert tm.n_retried_pairs == 0, "pairs left wfa_duo_kernel: the records below would come from the retry kernel"
    want = O.align_batch(O.make_params(*pen, global_alignment=True, adaptive=ad), *data, n_threads=8)
    assert np.array_equal(got.status, want.status) and not np.any(got.status)
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert np.array_equal(a, b), f"pen={pen} ad={ad}: field {f} differs at pairs {np.nonzero(a != b)[0][:8]}"
    for i in range(n):
        assert np.array_equal(got.pair_ops(i), want.pair_ops(i)), f"pen={pen} ad={ad}: CIGAR differs at pair {i}"
