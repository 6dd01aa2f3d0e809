"""The pileup (include/wfa_hip.h: wfahip_pileup_device and its siblings) restated in Python with np.add.at over exact integers,
written from the rule's text and sharing no code with wfa_amd/csrc/wfa_pile.hpp: tests/test_pile_abi.py holds the host entries against
it, tests/test_pile_gpu.py the kernels.  It works over the dicts of check_cases.arrays() -- status, ops_off, ops_len, ops, qbegin, qend,
tbegin, tend and seqs = (blob or words, q_off, q_len, t_off, t_len[, q_rc]) -- and over real results through
check_cases.from_results().  Also here: set_aside(), which does to such a dict what a caller does with the check's d_pass, and the
shared-target batch both test files run over."""
import functools

import numpy as np

import check_cases as X
from altext_pk_cases import pack_seq, packed_words, revcomp

OK = 0
M32 = 0xFFFFFFFF
WORDS = 8
A, C, T, G, OTHER, GAP, EXTRA, EXTRA_BASES = range(8)
NAMES = ("A", "C", "T", "G", "OTHER", "GAP", "EXTRA", "EXTRA_BASES")
SET_ASIDE = 16     # WFAHIP_PAIR_CHECK_FAILED: what d_pass holds for a pair with a flag of the mask
POISON = (1 << 63) + 12345

_WORD_OF_BYTE = np.full(256, OTHER, np.int64)
for _b in b"ACGTacgt":
    _WORD_OF_BYTE[_b] = (_b >> 1) & 3


def _split(op):
    return int(op) >> 32, int(op) & M32


def pair_plan(a, i, only_aligned, packed=False, size=None):
    """what pair i of the dict does to a pileup: None -- it adds nothing and none of its offsets is looked at --, False -- it fails
    a check, the call is WFAHIP_ERR_BAD_ARG --, or (ops, query words of its window, T0, target bases of its window, swept): the ops
    that count as (letter, count), the counter word of every base of the query's window, the coordinate of the target window's
    first base, and whether the pair has a column"""
    if int(a["status"][i]) != OK:
        return None
    seqs, q_off, q_len, t_off, t_len = a["seqs"][:5]
    q_rc = a["seqs"][5] if packed and len(a["seqs"]) > 5 else None
    size = len(seqs) if size is None else size
    cap = len(a["ops"])
    L, off = int(a["ops_len"][i]), int(a["ops_off"][i])
    if L > cap or off > cap - L:
        return False
    if L == 0:
        return None
    ops = [_split(o) for o in a["ops"][off:off + L]]
    if only_aligned:
        m = [k for k, (l, _) in enumerate(ops) if l == ord("M")]
        if not m:
            return None
        ops = ops[m[0]:m[-1] + 1]
    cols = sum(n for l, n in ops if l in b"MXIDH")
    q_used = sum(n for l, n in ops if l in b"MXDH")
    t_used = sum(n for l, n in ops if l in b"MXI")
    if packed and cols == 0:
        return None
    qo, ql, to, tl = int(q_off[i]), int(q_len[i]), int(t_off[i]), int(t_len[i])
    need = packed_words if packed else (lambda n: n)
    if any(o > size or need(ln) > size - o for o, ln in ((qo, ql), (to, tl))):
        return False
    q_at, q_n, t_at, t_n = 0, ql, 0, tl
    if only_aligned:
        qb, qe, tb, te = (int(a[k][i]) for k in ("qbegin", "qend", "tbegin", "tend"))
        if not (qb >= 1 and qb - 1 <= qe <= ql and tb >= 1 and tb - 1 <= te <= tl):
            return False
        q_at, q_n, t_at, t_n = qb - 1, qe - (qb - 1), tb - 1, te - (tb - 1)
    if q_used > q_n or t_used > t_n:
        return False
    if cols == 0:
        return (ops, None, 0, t_n, False)
    if packed:
        codes = X.unpack_codes(seqs, qo, ql, q_rc is not None and bool(q_rc[i]))
        q_words = codes[q_at:q_at + q_n].astype(np.int64)
        T0 = 16 * to + t_at
    else:
        q_words = _WORD_OF_BYTE[seqs[qo + q_at:qo + q_at + q_n]]
        T0 = to + t_at
    return (ops, q_words, T0, t_n, True)


def restate(a, pile_at, pile_n, only_aligned, packed=False, size=None, into=None):
    """(counts uint32 [pile_n, 8], n_piled) as the entries must leave them -- added to `into` when given --, or None where they
    must return WFAHIP_ERR_BAD_ARG"""
    plans = [pair_plan(a, i, only_aligned, packed, size) for i in range(len(a["status"]))]
    if any(p is False for p in plans):
        return None
    counts = np.zeros((pile_n, WORDS), np.uint64) if into is None else into.astype(np.uint64)
    n_piled = 0
    for p in plans:
        if p is None or not p[4]:
            continue
        n_piled += 1
        ops, q_words, T0, t_n, _ = p
        qs = ts = 0
        for letter, n in ops:
            if letter in b"MXI":
                lo, hi = max(0, pile_at - (T0 + ts)), min(n, pile_at + pile_n - (T0 + ts))   # the op's columns inside the window
                if lo < hi:
                    idx = np.arange(T0 + ts + lo - pile_at, T0 + ts + hi - pile_at, dtype=np.int64)
                    word = np.full(hi - lo, GAP, np.int64) if letter == ord("I") else q_words[qs + lo:qs + hi]
                    np.add.at(counts, (idx, word), 1)
            elif letter == ord("D") and n > 0 and t_n > 0:
                P = T0 + max(ts, 1) - 1
                if pile_at <= P < pile_at + pile_n:
                    np.add.at(counts, ([P - pile_at] * 2, [EXTRA, EXTRA_BASES]), [1, n])
            qs += n if letter in b"MXDH" else 0
            ts += n if letter in b"MXI" else 0
    return (counts & np.uint64(M32)).astype(np.uint32), n_piled


def set_aside(a, only_aligned, packed=False):
    """a copy of the dict in which every pair that fails a check has the status WFAHIP_PAIR_CHECK_FAILED (in status and in the
    records), as a caller makes it from the check's d_pass; all offsets of every pair that is not OK are poisoned.  Returns (the copy,
    the indices set aside)."""
    b = dict(a)
    b["status"] = a["status"].copy()
    bad = [i for i in range(len(a["status"])) if pair_plan(a, i, only_aligned, packed) is False]
    b["status"][bad] = SET_ASIDE
    seqs = [np.array(x) for x in a["seqs"]]
    off_ok = b["status"] == OK
    seqs[1][~off_ok] = POISON
    seqs[3][~off_ok] = POISON
    b["seqs"] = tuple(seqs)
    if "rec" in a:
        b["rec"] = a["rec"].copy()
        b["rec"][:, 0] = b["status"].view(np.uint32)
    return b, bad


def span(a, packed=False):
    """(pile_at, pile_n) of a window over everything the sequences of the dict's OK pairs can touch"""
    seqs = a["seqs"][0]
    return 0, (16 if packed else 1) * len(seqs)


# ---- the shared-target batch: N_TARGETS targets of TARGET_LEN bases, DEPTH mutated reads of each, t_off repeated

N_TARGETS, TARGET_LEN, DEPTH = 8, 300, 40


def _mutate(t, rng, rate=0.06):
    out = bytearray()
    for b in t:
        r = rng.random()
        if r < rate / 3:
            continue                                              # the read lacks the base
        if r < 2 * rate / 3:
            out.append(b"ACGT"[(b"ACGT".index(b) + int(rng.integers(1, 4))) % 4])
            continue
        out.append(b)
        if r < rate:
            out += bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 4))).astype(np.uint8))   # the read has extra bases
    return bytes(out)


@functools.lru_cache(maxsize=None)
def shared_targets(seed=41):
    """dict(bytes=check_cases dict over a blob, words=the same results over 2-bit words with every second query flagged, depth,
    targets=[(byte offset, word offset, length)]): aligned once a process by the CPU oracle (global, 4/6/2, no wf-adaptive), then
    left unchanged"""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    targets = [bytes(rng.choice(list(b"ACGT"), TARGET_LEN).astype(np.uint8)) for _ in range(N_TARGETS)]
    reads = [[_mutate(t, rng) for _ in range(DEPTH)] for t in targets]
    n = N_TARGETS * DEPTH
    q_off, t_off, q_woff, t_woff = (np.zeros(n, np.uint64) for _ in range(4))
    q_len, t_len = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    q_rc = (np.arange(n) & 1).astype(np.uint8)
    blob, words, at, wat, where = [], [], 3, 0, []                 # (the first target at an odd byte offset)
    blob.append(b"NNN")
    for k, t in enumerate(targets):
        where.append((at, wat, len(t)))
        for j in range(DEPTH):
            t_off[k * DEPTH + j], t_woff[k * DEPTH + j], t_len[k * DEPTH + j] = at, wat, len(t)
        blob.append(t)
        at += len(t)
        w = pack_seq(t)
        words.append(w)
        wat += len(w)
    for k in range(N_TARGETS):
        for j in range(DEPTH):
            i, q = k * DEPTH + j, reads[k][j]
            q_off[i], q_woff[i], q_len[i] = at, wat, len(q)
            blob.append(q)
            at += len(q)
            w = pack_seq(revcomp(q) if q_rc[i] else q)
            words.append(w)
            wat += len(w)
    blob = np.frombuffer(b"".join(blob), np.uint8)
    words = np.concatenate(words)
    w = O.align_batch(O.make_params(4, 6, 2, global_alignment=True), blob, q_off, q_len, t_off, t_len, n_threads=8)
    by = X.from_results(w, (blob, q_off, q_len, t_off, t_len))
    pk = X.from_results(w, (words, q_woff, q_len, t_woff, t_len, q_rc))
    for d in (by, pk):
        for v in list(d.values()) + list(d["seqs"]):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return dict(bytes=by, words=pk, depth=DEPTH, targets=where, oracle=w)
