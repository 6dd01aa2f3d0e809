"""Batches on which the start of a semi-global backtrace is what can go wrong (a helper module, no test).

The reference picks that start in backtraceStartPosistion (wfa.go:270-375): for every score from the one the forward pass
stopped at down to 0 it scans M[s] from the final diagonal Ak = m - n downwards, then from Ak + 1 upwards; a scan ends at the
first cell that leaves the matrix or lies on the last row or column; a hit counts only at a score <= the best so far, and the
upward scan overrides the downward one at equal score.  wfa_amd.generate_pairs -- what the tests of the long-pair kernels run on
-- gives reads of near-equal length whose alignment ends on or next to Ak at the final score, where "Ak at the last score" is
nearly always the answer.  These pairs end somewhere else.

ends_free() and ends_adapt() each build one batch (once per process) in the layout of wfa_amd.make_blob -- every sequence starts
on a 16-byte boundary -- and return (data, kinds): data = (blob, q_off, q_len, t_off, t_len), read-only; kinds[i] names how pair
i was made.  Every byte is A, C, G or T and every sequence has at least one base.  ends_free() is for wf-adaptive off: reads of
120 to 6 200 bases, n + m up to about 9 000.  ends_adapt() is for wf-adaptive 10/50/1: |m - n| <= 12 for every pair (beyond
MaxDistDiff the reference's first reduce cuts Ak off and the alignment runs on for thousands of scores), about half of the pairs
1 000 to 1 300 bases and half 2 060 to 2 300, whose n + m - 1 seeds span more than 4 096 diagonals.  The kinds, each both ways
round ("/q": the longer or the suffix read is the query):
  * "contained fl=.. fr=..": a core with about 1 % edits (substitutions, one 1-base insertion and one 1-base deletion) inside
    the other read behind fl random bases and before fr.  The alignment ends on diagonal +-fl while Ak = +-(fl + fr): the row
    that first touches the last row or column does so many scores before M[s][Ak] gets there (a gap of fr bases later).
    Free: fl in {0, 1, 2, 50, 600} x fr in {0, 1, 37}; adapt: fl, fr in {0, 1, 5, 12} with fl + fr <= 12, at both lengths;
  * "far fl=.. fr=.." (free): the same with fl in {0, 1, 300} and fr in {4 095, 4 096, 4 097, 4 500} -- the hit lies a whole
    stripe of wfa_teamc_kernel (TC_STRIPE = 4 096 diagonals) or more from Ak; where the longer read stays within 6 200 bases the
    core has 2 050 to 2 090, so that n + m - 1 > 8 192: three stripes.  Two more contained pairs (a 4 200-base core, flanks of
    300) have the widest rows of the batch, about 9 000 diagonals;
  * "edge b=.. d=.." (free): contained pairs whose Ak lies d diagonals past the last diagonal of stripe b (d = -1, 0: in that
    stripe; 1, 2: in the next one) of a team of three with team_slack = 1024 -- see "The axis" below;
  * "overhang c=..": a suffix of one read against a prefix of the other, equal lengths, the ends c bases apart
    (free: 1, 17, 300; adapt: 1, 5, 12);
  * "repeat unit=.. d=.. subs=..": both reads the same repeat of A, AC, ACG or of a random 500-base unit ("R500", the shorter
    read ending in a partial copy), lengths d apart (free: 0, 1, 50, 1 500; adapt: 0, 1, 12), with 0 and with 1 or 2
    substitutions by a base the unit does not contain (R500 holds all four: by another base) -- every diagonal a period apart
    ties, and the scans meet hits on many of them;
  * "identical", "equal": q == t (one of them 120 bases), and equal lengths with edits;
  * "unrelated" (free): four pairs of random reads of 120 to 500 bases;
  * "small fl=.. fr=..": contained pairs with a core of only 150 to 240 bases.  Under wf-adaptive the rows between the hit and
    the last score are the narrow ones that wave mode (rows of <= 64 diagonals) steps.
tests/test_semi_global_ends.py proves from the oracle alone that the batches hold enough pairs of every class the GPU tests are
about (K < Ak, K > Ak, K == Ak, score below the last score, either end rule, both length orders, far hits, three stripes).

The axis.  wfa_teamc_kernel (wfa_teamc.hpp) keeps the rows of a team of T workgroups on a fixed axis of diagonals: workgroup b
owns [KB + b S, KB + (b + 1) S).  When a row [lo, hi] of W diagonals enters the team's stripe mode it sets
    S  = min(4 096, round_up_64(ceil((W + 2 min(team_slack, 256)) / T)))
    KB = lo - min((T S - W) / 2, team_slack)          (integer division)
and leaves the axis alone while the rows stay inside it.  The first row of a semi-global pair is its seeds, lo = -(n - 1),
hi = m - 1, W = n + m - 1, and without wf-adaptive no later row is narrower or lies elsewhere: the axis never moves.  A row of
more than 4 094 diagonals is a team's at every team_solo_max.  axis(n, m, T, slack) below is that rule; _edge_lengths() walks the
lengths until Ak = m - n = KB + (b + 1) S - 1 + d.  With T = 3 and slack = 1 024 that is m about 2 n + 257 for the edge between
stripes 1 and 2 (the read in a longer target) and m about n / 2 - 129 for the edge between stripes 0 and 1 (a target in a
longer query)."""
import functools

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
TC_STRIPE = 4096  # wfa_ladder.hpp


def axis(n, m, T=3, slack=1024):
    """(KB, S) of wfa_teamc_kernel's first stripe-mode axis for a semi-global pair of n x m bases (the module docstring)"""
    W = n + m - 1
    S = min(TC_STRIPE, (-(-(W + 2 * min(slack, 256)) // T) + 63) & ~63)
    return -(n - 1) - min((T * S - W) // 2, slack), S


def _edge_lengths(core, b, d, T=3, slack=1024):
    """(n, m) with min(n, m) = core and Ak = m - n exactly d diagonals past the last one of stripe b"""
    for other in range(core + 1, 6200):
        n, m = (core, other) if b == 1 else (other, core)
        KB, S = axis(n, m, T, slack)
        if m - n == KB + (b + 1) * S - 1 + d:
            return n, m
    raise AssertionError(("no lengths put Ak there", core, b, d))


def _rand(rng, L):
    return ACGT[rng.integers(0, 4, L)]


def _other(rng, base):
    """one of the three bases that differ from `base`"""
    return ACGT[(int(np.nonzero(ACGT == base)[0][0]) + 1 + int(rng.integers(0, 3))) % 4]


def _edit(rng, seq, rate=0.01):
    """a copy of the same length with about rate * len substitutions and, from 400 bases, one 1-base insertion and one 1-base
    deletion; nothing within 12 bases of either end"""
    s = seq.copy()
    L = len(s)
    if rate <= 0 or L < 40:
        return s
    for p in rng.choice(np.arange(12, L - 12), max(1, int(round(L * rate))), replace=False):
        s[p] = _other(rng, s[p])
    if L >= 400:
        a, b = sorted(int(p) for p in rng.choice(np.arange(20, L - 20), 2, replace=False))
        s = np.delete(np.insert(s, a, _other(rng, s[a])), b + 1)
    assert len(s) == L
    return s


def _contained(rng, L, fl, fr, swap, rate=0.01):
    core = _rand(rng, L)
    outer = np.concatenate([_rand(rng, fl), _edit(rng, core, rate), _rand(rng, fr)])
    return (outer, core) if swap else (core, outer)


def _overhang(rng, L, c, swap):
    x = _rand(rng, L + c)
    a, b = x[c:].copy(), _edit(rng, x)[:L]
    return (b, a) if swap else (a, b)


def _repeat(rng, unit, n, d, n_sub, swap):
    """the shorter read has n bases, the longer n + d and the substitutions"""
    if unit == "R500":
        u = _rand(rng, 500)
    else:
        u = np.frombuffer(unit.encode(), dtype=np.uint8)
    a = np.tile(u, (n + d) // len(u) + 1)[:n].copy()
    b = np.tile(u, (n + d) // len(u) + 1)[:n + d].copy()
    foreign = [x for x in ACGT if x not in u]
    for p in rng.choice(np.arange(10, n - 10), n_sub, replace=False):
        b[p] = foreign[0] if foreign else _other(rng, b[p])
    return (b, a) if swap else (a, b)


def _blob(pairs):
    """the layout of wfa_amd.make_blob: q then t, each from a 16-byte boundary; read-only"""
    q_len = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
    t_len = np.array([len(t) for _, t in pairs], dtype=np.uint32)
    q_cap = (q_len.astype(np.uint64) + 15) & ~np.uint64(15)
    t_cap = (t_len.astype(np.uint64) + 15) & ~np.uint64(15)
    tot = q_cap + t_cap
    q_off = np.concatenate([[0], np.cumsum(tot)[:-1]]).astype(np.uint64)
    t_off = q_off + q_cap
    blob = np.zeros(int(tot.sum()), dtype=np.uint8)
    for i, (q, t) in enumerate(pairs):
        blob[int(q_off[i]):int(q_off[i]) + len(q)] = q
        blob[int(t_off[i]):int(t_off[i]) + len(t)] = t
    data = (blob, q_off, q_len, t_off, t_len)
    for a in data:
        a.setflags(write=False)
    return data


class _Batch:
    def __init__(self, seed):
        self.rng, self.pairs, self.kinds = np.random.default_rng(seed), [], []

    def add(self, kind, pair, swap=False):
        self.pairs.append(pair), self.kinds.append(kind + ("/q" if swap else ""))

    def done(self):
        return _blob(self.pairs), tuple(self.kinds)


@functools.lru_cache(maxsize=None)
def ends_free():
    B = _Batch(20250601)
    rng = B.rng
    for fl in (0, 1, 2, 50, 600):
        for fr in (0, 1, 37):
            for swap in (False, True):
                B.add(f"contained fl={fl} fr={fr}", _contained(rng, int(rng.integers(1200, 1501)), fl, fr, swap), swap)
    for i, (fl, fr) in enumerate((fl, fr) for fl in (0, 1, 300) for fr in (4095, 4096, 4097, 4500)):
        swap = i % 2 == 1
        L = int(rng.integers(2050, 2091)) if fl + fr <= 4100 else int(rng.integers(1200, 1401))  # (no read beyond 6 200 bases)
        B.add(f"far fl={fl} fr={fr}", _contained(rng, L, fl, fr, swap), swap)
    for swap in (False, True):  # the widest rows of the batch: about 9 000 diagonals
        B.add("contained fl=300 fr=300", _contained(rng, 4200, 300, 300, swap), swap)
    for b in (0, 1):
        for d in (-1, 0, 1, 2):
            n, m = _edge_lengths(1300 + 7 * d, b, d)
            core, flanks = min(n, m), abs(m - n)
            B.add(f"edge b={b} d={d}", _contained(rng, core, 1, flanks - 1, b == 0), b == 0)
    for c in (1, 17, 300):
        for swap in (False, True):
            B.add(f"overhang c={c}", _overhang(rng, 2000 if c == 300 else int(rng.integers(1200, 1501)), c, swap), swap)
    i = 0
    for unit in ("A", "AC", "ACG", "R500"):
        for d in (0, 1, 50, 1500):
            for subs in (0, 1 + i % 2):
                n = 1077 if unit == "R500" else int(rng.integers(1000, 1501))
                B.add(f"repeat unit={unit} d={d} subs={subs}", _repeat(rng, unit, n, d, subs, i % 3 == 1), i % 3 == 1)
                i += 1
    x = _rand(rng, 120)
    B.add("identical", (x.copy(), x))
    x = _rand(rng, 1400)
    B.add("identical", (x.copy(), x))
    for L in (500, 1200, 1500, 2100):
        x = _rand(rng, L)
        B.add("equal", (_edit(rng, x, 0.02), x))
    for n, m in ((120, 500), (500, 120), (300, 500), (400, 400)):
        B.add("unrelated", (_rand(rng, n), _rand(rng, m)))
    for i, (fl, fr) in enumerate(((0, 1), (0, 37), (1, 37), (2, 1), (50, 37), (0, 300), (1, 300), (50, 1))):
        swap = i % 2 == 1
        B.add(f"small fl={fl} fr={fr}", _contained(rng, int(rng.integers(150, 241)), fl, fr, swap, rate=0.02), swap)
    return B.done()


@functools.lru_cache(maxsize=None)
def ends_adapt():
    B = _Batch(20250602)
    rng = B.rng
    length = lambda big, room=0: int(rng.integers(2060, 2281 - room)) if big else int(rng.integers(1000, 1281 - room))
    flanks = [(fl, fr) for fl in (0, 1, 5, 12) for fr in (0, 1, 5, 12) if fl + fr <= 12]
    for big in (False, True):
        for fl, fr in flanks:
            for swap in (False, True):
                B.add(f"contained fl={fl} fr={fr}", _contained(rng, length(big, 12), fl, fr, swap), swap)
    for big in (False, True):
        for c in (1, 5, 12):
            for swap in (False, True):
                B.add(f"overhang c={c}", _overhang(rng, length(big), c, swap), swap)
    i = 0
    for unit in ("A", "AC", "ACG", "R500"):
        for d in (0, 1, 12):
            for subs in (0, 1 + i % 2):
                n = (2077 if i % 4 < 2 else 1077) if unit == "R500" else length(i % 4 < 2, 12)
                B.add(f"repeat unit={unit} d={d} subs={subs}", _repeat(rng, unit, n, d, subs, i % 3 == 1), i % 3 == 1)
                i += 1
    x = _rand(rng, 120)
    B.add("identical", (x.copy(), x))
    for big in (False, True):
        x = _rand(rng, length(big))
        B.add("identical", (x.copy(), x))
        for _ in range(2):
            x = _rand(rng, length(big))
            B.add("equal", (_edit(rng, x, 0.02), x))
    for i, (fl, fr) in enumerate(((0, 1), (0, 5), (0, 12), (1, 5), (5, 5), (1, 1), (5, 1), (0, 12))):
        swap = i % 2 == 1
        B.add(f"small fl={fl} fr={fr}", _contained(rng, int(rng.integers(150, 241)), fl, fr, swap, rate=0.02), swap)
    return B.done()
