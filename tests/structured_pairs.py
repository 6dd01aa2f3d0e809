"""Batches on which WF_EXTEND, the read ends and tied next() sources are what can go wrong (a helper module, no test).

structured_batch(n_pairs, l_min, l_max, seed, wide_every=0) builds one batch (once per parameter set) in the layout of wfa_amd.make_blob
-- every sequence starts on a 16-byte boundary -- and returns (data, kinds): data = (blob, q_off, q_len, t_off, t_len), read-only;
kinds[i] names how pair i was built.  The kinds are dealt by index (i mod 10) as tests/test_duo_extend_gpu.py deals them:
  * "ident" (i mod 10 == 0): q == t, one run over the whole read;
  * "runs" (1, 2, 4, 6, 8, 9): t random, q = t with a substitution at text offset P - 1, an exact run of `run` bases from P, a
    substitution, then at most two further runs drawn from RUNS -- three runs at most, four cuts.  RUNS is one base either side of
    the first 16-base window and of each 32-base round behind it; P = 16 + start_mod, start_mod 0 or 15; shift 0 / +1 / -1: one
    base deleted from / inserted into q at position 5, so the runs lie on the main diagonal or one either side of it and the two
    sequences' windows start at different bit positions of their words.  The plan (run, start_mod, shift) is walked exhaustively;
  * "end" (3, 7): the shorter read is a prefix of the longer one, d = 1 or 3 bases shorter, with one substitution run + 1 bases
    before its end -- the last run ends exactly on the shorter read's last base, either read the shorter one: the extension's
    window reads the pad word and beyond, and only the clamp by the bases that are left keeps padding from counting;
  * "rep" (5): both reads the same repeat of unit A, C, AC, GT or ACG, lengths 0, 1, 2 or 4 apart, 0 or 2 substitutions by a base
    the unit does not contain, either read the query: every diagonal of a row runs long in the same step, and the sources of
    next() tie;
  * "wide" (only with wide_every = w > 0: i mod w == w // 2, whatever i mod 10 would have dealt): t random, q = t with ten
    substitutions spread evenly over the read, as tests/test_duo_extend_gpu.py builds them -- score 40 at 4/6/2, where without
    wf-adaptive the band outgrows what wfa_duo_kernel gives a narrow pair.  wide_every = 0 draws nothing from the generator:
    the batches without wide pairs are what they were before the argument existed.
What holds for every batch (its wide pairs aside, which have ten substitutions and no gap):
  * the LONGER read of a pair has l_min .. l_max bases -- no read is longer than l_max; the shorter one is at most 4 bases shorter
    (max |m - n| = 4) -- and in every tenth pair of each kind the longer read has exactly l_max bases;
  * every byte is A, C, G or T;
  * a pair differs by at most four substitutions and one 1-base gap ("runs"), one substitution and a 3-base gap ("end"), or two
    substitutions and a 4-base gap ("rep"): at 4/6/2 the global score is at most 24.
tests/test_structured_pairs.py proves from the oracle alone, for the batches and penalties the GPU tests use, that every row
next() computes spans at most 28 diagonals and every stored M cell lies within 14 diagonals of the main one, wf-adaptive on or
off -- and what it proves of the wide pairs' rows instead.

The seam batches put these pairs where the router's integer arithmetic changes a kernel or a layout (wfa_host.hip:
seq_words = (max_len + 15) / 16 + 1; wfa_duo_kernel's slot PW = 4 + 2 * ((seq_words + 1) & ~1) words, 256 / PW pairs per fetch).
Every DUO_SEAMS batch spans 16 bases, l_max a multiple of 16: one seq_words class, the longest reads filling its last word."""
import functools

import numpy as np

RUNS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
PLAN = tuple((r, a, s) for r in RUNS for a in (0, 15) for s in (0, 1, -1))
ENDS = tuple((r, d, qs) for r in RUNS for d in (1, 3) for qs in (True, False))
REPS = tuple((u, d, ns) for u in (b"A", b"C", b"AC", b"GT", b"ACG") for d in (0, 1, 2, 4) for ns in (0, 2))
# the batches the tests use, as arguments of structured_batch: (n_pairs, l_min, l_max, seed)
SHORT = (400, 150, 199, 20250301)     # under 200 bases: the 8-lane short-read instance of the blocked kernel takes them
LANE = (400, 224, 240, 20250302)      # up to wfa_lane_kernel's 240 bases; (15 packed words of sequence and the pad word)
LANE_EDGE = {L: (64, L, L, 20250303 + L) for L in (239, 240, 241)}  # every longer read at, one under and one over the limit
SCORE_EDGE = (64, 2040, 2047, 20250304)  # up against SCORE_MAX_LEN = 2 047 and the 16-bit ring offsets of the score kernels
SCORE_LONG = (64, 2048, 2060, 20250305)  # just past it: wfa_score_long_kernel's
# (n_pairs, l_min, l_max, seed, wide_every) -- wfa_duo_kernel: the 16-base class at both ends of every pairs-per-fetch class (8, 7, 7,
# 6, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1 pairs); 4 099 pairs: not divisible by 2 .. 8, the queue ends on a partial fetch of every size
DUO_CLASSES = ((193, 208), (209, 224), (225, 240), (241, 256), (257, 272), (273, 288), (321, 336), (337, 352), (449, 464), (465, 480),
               (609, 624), (625, 640), (961, 976), (977, 992), (1985, 2000))
DUO_SEAMS = {c: (4099, c[0], c[1], 20250400 + c[1], 50) for c in DUO_CLASSES}
# wfa_blk_kernel, 16 lanes: one base past wfa_duo_kernel's 2 000; up to long_min_len = 4 000; up to lds_d = 20 464 of 20 480 bytes
# (option long = 0); and the far side of that gate
BLK_SEAMS = {(2001, 2016): (209, 2001, 2016, 20250501), (3985, 4000): (64, 3985, 4000, 20250502),
             (10193, 10208): (64, 10193, 10208, 20250503), (10209, 10224): (16, 10209, 10224, 20250504)}
LONG_SEAM = (64, 4001, 4016, 20250505)  # the shortest reads of the sliding-window kernels: the default window repositions once
S200 = (209, 200, 200, 20250506)        # one base past the short-read instance's max_len < 200


def _other(base):
    """a base that differs from `base` (A -> C -> G -> T -> A)"""
    return ACGT[(int(np.nonzero(ACGT == base)[0][0]) + 1) % 4]


def _subst(seq, pos):
    seq[pos] = _other(seq[pos])


def _runs_pair(rng, L, run, start_mod, shift):
    """the longer read has L bases: t when shift >= 0 (q = t, or t less one base), q when shift < 0 (t plus one base)"""
    Lt = L - 1 if shift < 0 else L
    t = ACGT[rng.integers(0, 4, Lt)]
    q = t.copy()
    P = 16 + start_mod
    cuts, pos = [P - 1], P + run
    for _ in range(1 + int(rng.integers(0, 3))):
        if pos >= Lt - 1:
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


def _end_pair(rng, L, run, d, q_short):
    long_ = ACGT[rng.integers(0, 4, L)]
    short = long_[:L - d].copy()
    _subst(short, len(short) - run - 1)
    return (short, long_) if q_short else (long_, short)


def _repeat_pair(rng, L, unit, d, n_sub):
    """L: the longer read"""
    u = np.frombuffer(unit, dtype=np.uint8)
    a = np.tile(u, L // len(u) + 2)[:L - d].copy()
    b = np.tile(u, L // len(u) + 2)[:L].copy()
    foreign = ACGT[[x not in u for x in ACGT]][0]
    if n_sub:
        for p in rng.choice(np.arange(10, L - d - 10), n_sub, replace=False):
            b[p] = foreign
    return (a, b) if rng.integers(0, 2) else (b, a)


def _wide_pair(rng, L):
    """ten substitutions, evenly spread (each within 5 bases of its place)"""
    t = ACGT[rng.integers(0, 4, L)]
    q = t.copy()
    for p in np.linspace(12, L - 12, 10).astype(int) + rng.integers(-5, 6, 10):
        _subst(q, int(p))
    return q, t


@functools.lru_cache(maxsize=None)
def structured_batch(n_pairs, l_min, l_max, seed, wide_every=0):
    assert 120 <= l_min <= l_max and wide_every >= 0
    rng = np.random.default_rng(seed)
    seen = {"ident": 0, "runs": 0, "end": 0, "rep": 0, "wide": 0}
    pairs, kinds = [], []
    for i in range(n_pairs):
        kind = {0: "ident", 3: "end", 7: "end", 5: "rep"}.get(i % 10, "runs")
        if wide_every and i % wide_every == wide_every // 2:
            kind = "wide"
        L = int(rng.integers(l_min, l_max + 1))
        if seen[kind] % 10 == 9:
            L = l_max
        j = seen[kind]
        seen[kind] += 1
        if kind == "ident":
            t = ACGT[rng.integers(0, 4, L)]
            pair = (t.copy(), t)
        elif kind == "end":
            pair = _end_pair(rng, L, *ENDS[j % len(ENDS)])
        elif kind == "rep":
            pair = _repeat_pair(rng, L, *REPS[j % len(REPS)])
        elif kind == "wide":
            pair = _wide_pair(rng, L)
        else:
            pair = _runs_pair(rng, L, *PLAN[(j * 7 + j // len(PLAN)) % len(PLAN)])
        pairs.append(pair), kinds.append(kind)
    # the layout of wfa_amd.make_blob: q then t, each from a 16-byte boundary
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
    return data, tuple(kinds)
