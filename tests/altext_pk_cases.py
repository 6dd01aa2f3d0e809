"""Packed words for the display-row entries that read them (tests/test_altext_packed_abi.py on the host renderer,
tests/test_altext_packed_gpu.py on the kernels).  A case is altext_cases' (status, [op words], query bytes, target bytes, qbegin,
qend, tbegin, tend) with ACGT sequences; its query bytes are the strand the record and the ops speak of, so a FLAGGED case is packed
as the reverse complement of its query bytes and the entry has to turn it back.  pack() scatters the sequences through one word
array; altext_cases.expected() on the same cases is the reference."""
import numpy as np

import altext_cases as A
import cigar_cases as K
from cigar_cases import OK, op  # noqa: F401

STALE_WOFF, STALE_LEN = (1 << 50) + 5, 123  # the words of a pair that renders nothing may lie anywhere: they are not read
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return bytes(b)[::-1].translate(_COMP)


def acgt(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()


def with_acgt(cases, seed=17):
    """the cases with their sequences replaced by random ACGT of the same lengths"""
    rng = np.random.default_rng(seed)
    return [(c[0], c[1], acgt(rng, len(c[2])), acgt(rng, len(c[3])), *c[4:]) for c in cases]


def packed_words(n):
    return (n + 15) // 16 + 1


def pack_seq(b, rng=None):
    """wfahip_packed_words(len(b)) words: 16 bases a word, code (ascii >> 1) & 3, then the pad word; the bits beyond the last base
    and the pad word zero, or random with an rng"""
    n, nw = len(b), packed_words(len(b))
    codes = np.zeros(16 * nw, np.uint64) if rng is None else rng.integers(0, 4, 16 * nw).astype(np.uint64)
    codes[:n] = (np.frombuffer(bytes(b), np.uint8) >> 1) & 3
    return (codes.reshape(nw, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


def renders(case):
    return case[0] == OK and bool(case[1])


def pack(cases, flags, seed=3, junk_tails=None, gaps=True):
    """(words uint32, q_woff uint64, q_len uint32, t_woff uint64, t_len uint32, q_rc uint8): the sequences in a shuffled order,
    0 to 2 junk words between them when gaps; a flagged query packed as its reverse complement; a case that renders nothing in either
    mode (not OK, or no op) gets stale offsets far outside the words.  junk_tails: a seed for random tail bits and pad words.  The
    LAST sequence ends exactly at the end of the words."""
    rng = np.random.default_rng(seed)
    tails = None if junk_tails is None else np.random.default_rng(junk_tails)
    n = len(cases)
    q_woff, t_woff = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    q_len, t_len = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    q_rc = np.array([1 if f else 0 for f in flags], np.uint8)
    assert len(q_rc) == n
    parts, at = [], 0
    for i in rng.permutation(n):
        st, ops, q, t = cases[i][:4]
        if not renders(cases[i]):
            q_woff[i] = t_woff[i] = STALE_WOFF
            q_len[i] = t_len[i] = STALE_LEN
            continue
        for seq, off, ln in ((t, t_woff, t_len), (revcomp(q) if q_rc[i] else q, q_woff, q_len)):
            if gaps:
                pad = int(rng.integers(0, 3))
                parts.append(rng.integers(0, 1 << 32, pad, dtype=np.uint64).astype(np.uint32))
                at += pad
            w = pack_seq(seq, tails)
            off[i], ln[i] = at, len(seq)
            parts.append(w)
            at += len(w)
    words = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return words, q_woff, q_len, t_woff, t_len, q_rc


def flags_of(kind, n):
    """'none' / 'all' / 'alt' -> n flags (alternating: pair 0 clear, pair 1 flagged, ..)"""
    return {"none": [0] * n, "all": [1] * n, "alt": [i & 1 for i in range(n)]}[kind]


def arrays(cases, flags, seed=11, junk_tails=None):
    """everything the host entry takes for a list of cases, as numpy arrays"""
    status, ops_off, ops_len, ops = K.lay_out([c[:2] for c in cases], seed=seed)
    return dict(status=status, ops_off=ops_off, ops_len=ops_len, ops=ops, win=A.windows(cases), pk=pack(cases, flags, seed=seed + 1, junk_tails=junk_tails))


# one pair for the checks, altext_cases.PAIR with ACGT sequences: trimmed it renders 4M over query bases [1, 5) and target bases [2, 6)
PAIR_Q, PAIR_T = b"GACGTCA", b"TTACGTGCA"
PAIR = (OK, A.PAIR_OPS, PAIR_Q, PAIR_T, 2, 5, 3, 6)   # the ops consume 7 query and 9 target bases
NOT_OK = (K.EMPTY, None, b"", b"", 0, 0, 0, 0)
NO_COLUMN = (OK, [op("~", 9), op("Z", 1)], b"", b"", 0, 0, 0, 0)   # OK, ops, but no column: its offsets are not looked at either


def one(flag=0, **kw):
    """arrays() of [PAIR, NOT_OK] with one thing changed; "n_words" is the number of words the entry is told of (default: all of
    them, and PAIR's later sequence ends exactly there)"""
    a = arrays([PAIR, NOT_OK], [flag, 0], seed=1)
    words, q_woff, q_len, t_woff, t_len, q_rc = a["pk"]
    qbegin, qend, tbegin, tend = a["win"]
    a["n_words"] = kw.pop("n_words", len(words))
    for k, v in kw.items():
        {"q_len": q_len, "t_len": t_len, "q_woff": q_woff, "t_woff": t_woff, "qbegin": qbegin, "qend": qend, "tbegin": tbegin, "tend": tend,
         "ops_off": a["ops_off"], "ops_len": a["ops_len"]}[k][0] = v
    return a
