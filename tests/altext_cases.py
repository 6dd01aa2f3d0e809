"""Synthetic records, ops and sequences for the display-row entries (tests/test_altext_abi.py on the host renderer,
tests/test_altext_gpu.py on the kernels): no alignment is involved, the entries take any records.  A case is (status, [op words],
query bytes, target bytes, qbegin, qend, tbegin, tend); cigar_cases.lay_out() scatters the ops, blob() scatters the sequences, and
expected() is AlignmentResult.AlignmentText of wfa_amd/aligner.py -- after an assertion that the ops fit the windows, because a
Python slice truncates where the reference would panic."""
import numpy as np

import cigar_cases as K
from cigar_cases import OK, op  # noqa: F401

STALE_SEQ_OFF, STALE_SEQ_LEN = (1 << 50) + 5, 123  # the sequence of a pair that renders nothing may lie anywhere: it is not read
Q_OF = {"M": 1, "X": 1, "D": 1, "H": 1}           # letters whose columns consume a query byte
T_OF = {"M": 1, "X": 1, "I": 1}                   # ... a target byte
# columns of the single-M pairs: the groups of 4 columns of the write kernel, its wave's 256 columns a sweep, powers of two
SINGLE_M = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
N_OPS = [0, 1, 63, 64, 65, 127, 128, 129, 200]    # the seams of the 64-op rounds


def consumed(ops):
    """(columns, query bytes, target bytes) of a list of op words"""
    c = q = t = 0
    for o in ops:
        letter, n = chr(int(o) >> 32) if (int(o) >> 32) < 256 else "?", int(o) & 0xFFFFFFFF
        q += n * Q_OF.get(letter, 0)
        t += n * T_OF.get(letter, 0)
        c += n if letter in "MXIDH" else 0
    return c, q, t


def trim(ops):
    m = [k for k, o in enumerate(ops) if (int(o) >> 32) == ord("M")]
    return (m[0], m[-1] + 1) if m else (0, 0)


def make(ops, rng, slack=0, status=OK):
    """a case whose sequences hold exactly the bases all ops consume, + slack bytes; with slack the trimmed windows are moved AWAY
    from where the trimmed-away ops end, so that only the record can say where they are"""
    ops = list(ops)
    _, tq, tt = consumed(ops)
    a, b = trim(ops)
    _, pq, pt = consumed(ops[:a])
    _, wq, wt = consumed(ops[a:b])
    q = rng.integers(0, 256, tq + slack, dtype=np.uint8).tobytes()
    t = rng.integers(0, 256, tt + slack, dtype=np.uint8).tobytes()
    if b == 0:
        return (status, ops, q, t, 0, 0, 0, 0)  # no M op: trimmed, nothing renders and the record's windows are not looked at

    def start(true_start, window, length):
        if not slack:
            return true_start
        choices = [s for s in (true_start + slack, true_start - 1, 0, length - window) if 0 <= s <= length - window and s != true_start]
        return choices[0]
    sq, st = start(pq, wq, len(q)), start(pt, wt, len(t))
    return (status, ops, q, t, sq + 1, sq + wq, st + 1, st + wt)


def cases(seed=7):
    rng = np.random.default_rng(seed)
    c = []
    base = K.base_cases()
    for k, (st, ops) in enumerate(base[3:12]):                                       # the trim cases, and ops_len 0
        c.append(make(ops, rng, slack=[0, 3, 7][k % 3]))
    for st, _ in base[12:]:                                                          # not OK: stale words, nothing rendered
        c.append((st, None, b"", b"", 0, 0, 0, 0))
    c.append(make([op("M", 3), op("~", 7), op("X", 0), op("M", 0), op("D", 2), op("I", 0), op("Z", 4000000000), op("M", 4)], rng, slack=2))
    c.append(make([op("~", 9), op("Z", 1)], rng))                                    # ops, but no column in either mode
    c.append(make([op("H", 5000), op("I", 3000), op("X", 2), op("M", 10), op("X", 1), op("M", 5), op("D", 2), op("I", 900)], rng, slack=11))
    c.append(make([op("I", 4100), op("H", 1), op("M", 1), op("H", 2600)], rng, slack=1))
    for n in N_OPS:                                                                  # counts 1 .. 20, every letter
        c.append(make([op("MXIDH"[int(rng.integers(0, 5))], int(rng.integers(1, 21))) for _ in range(n)], rng, slack=n % 2))
    for m_at in ((0, 199), (64, 128), (63,)):                                        # the only M ops at the rounds' seams
        ops = [op("M" if k in m_at else "XIDH"[int(rng.integers(0, 4))], int(rng.integers(1, 21))) for k in range(200)]
        c.append(make(ops, rng, slack=5))
    for n in SINGLE_M:
        c.append(make([op("M", n)], rng))
    c.append(make([op("X", 1), op("M", 70000), op("I", 3)], rng))                    # one op of 70 000 columns
    c.append(make([op("D", 70001)], rng))
    return c


def blob(cases_, seed=3):
    """(blob uint8, q_off uint64, q_len uint32, t_off uint64, t_len uint32): the sequences in a shuffled order with junk bytes
    between them, the k-th placed at an offset of residue k mod 16; a case that renders nothing in either mode (not OK, or no
    op) gets stale offsets far outside the blob"""
    rng = np.random.default_rng(seed)
    n = len(cases_)
    q_off, t_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    q_len, t_len = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    parts, at, placed = [], 0, 0
    for i in rng.permutation(n):
        st, ops, q, t = cases_[i][:4]
        if st != OK or not ops:
            q_off[i] = t_off[i] = STALE_SEQ_OFF
            q_len[i] = t_len[i] = STALE_SEQ_LEN
            continue
        for seq, off, ln in ((t, t_off, t_len), (q, q_off, q_len)):
            pad = (placed % 16 - at) % 16 + 16 * int(rng.integers(0, 2))
            parts.append(rng.integers(0, 256, pad, dtype=np.uint8).tobytes())
            at += pad
            off[i], ln[i] = at, len(seq)
            parts.append(seq)
            at += len(seq)
            placed += 1
    return np.frombuffer(b"".join(parts), np.uint8).copy(), q_off, q_len, t_off, t_len


def windows(cases_, seed=4):
    """(qbegin, qend, tbegin, tend) int32: the cases' values; junk for a case that is not OK"""
    rng = np.random.default_rng(seed)
    w = np.array([c[4:8] for c in cases_], np.int32).reshape(len(cases_), 4)
    for i, c in enumerate(cases_):
        if c[0] != OK:
            w[i] = rng.integers(-(1 << 31), 1 << 31, 4)
    return w[:, 0].copy(), w[:, 1].copy(), w[:, 2].copy(), w[:, 3].copy()


def records(status, ops_off, ops_len, win):
    """device records: cigar_cases.records' junk-filled words with the windows in TBEGIN, TEND, QBEGIN, QEND (words 2 .. 5)"""
    rec = K.records(status, ops_off, ops_len)
    qbegin, qend, tbegin, tend = win
    rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5] = tbegin.view(np.uint32), tend.view(np.uint32), qbegin.view(np.uint32), qend.view(np.uint32)
    return rec


def rows_of(case, only_aligned):
    """the three rows AlignmentResult.AlignmentText gives for a case (empty for a case that is not OK)"""
    import wfa_amd
    st, ops, q, t, qbegin, qend, tbegin, tend = case
    if st != OK or not ops:
        return b"", b"", b""
    if only_aligned:
        a, b = trim(ops)
        if b == 0:
            return b"", b"", b""
        _, wq, wt = consumed(ops[a:b])
        assert 1 <= qbegin and qbegin - 1 <= qend <= len(q) and wq <= qend - qbegin + 1
        assert 1 <= tbegin and tbegin - 1 <= tend <= len(t) and wt <= tend - tbegin + 1
    else:
        _, wq, wt = consumed(ops)
        assert wq <= len(q) and wt <= len(t)
    r = wfa_amd.AlignmentResult(Ops=list(ops), QBegin=qbegin, QEnd=qend, TBegin=tbegin, TEnd=tend)
    Q, A, T = r.AlignmentText(q, t, bool(only_aligned))
    assert len(Q) == len(A) == len(T)
    return Q, A, T


def expected(cases_, only_aligned):
    """(q_row, a_row, t_row uint8, off uint64 [n + 1]) as the entries must return them; a case object that occurs again is
    rendered once"""
    seen = {}
    rows = []
    for c in cases_:
        if id(c) not in seen:
            seen[id(c)] = rows_of(c, only_aligned)
        rows.append(seen[id(c)])
    off = np.zeros(len(rows) + 1, np.uint64)
    if rows:
        off[1:] = np.cumsum([len(r[0]) for r in rows], dtype=np.uint64)
    planes = [np.frombuffer(b"".join(r[k] for r in rows), np.uint8) for k in range(3)]
    return planes[0], planes[1], planes[2], off


def arrays(cases, seed=11):
    """everything the host entry takes for a list of cases, as numpy arrays"""
    status, ops_off, ops_len, ops = K.lay_out([c[:2] for c in cases], seed=seed)
    return dict(status=status, ops_off=ops_off, ops_len=ops_len, ops=ops, win=windows(cases), seqs=blob(cases))


# one pair for the checks: trimmed it renders 4M over query bytes [1, 5) and target bytes [2, 6)
PAIR_Q, PAIR_T = b"qACGTxy", b"ttACGTzuv"
PAIR_OPS = [op("H", 1), op("I", 2), op("M", 4), op("X", 1), op("D", 1), op("I", 2)]   # consumes 7 query and 9 target bytes
PAIR = (OK, PAIR_OPS, PAIR_Q, PAIR_T, 2, 5, 3, 6)


def one(**kw):
    """arrays() of PAIR (+ a pair that is not OK) with one thing changed"""
    a = arrays([PAIR, (K.EMPTY, None, b"", b"", 0, 0, 0, 0)], seed=1)
    blob, q_off, q_len, t_off, t_len = a["seqs"]
    qbegin, qend, tbegin, tend = a["win"]
    for k, v in kw.items():
        {"q_len": q_len, "t_len": t_len, "q_off": q_off, "t_off": t_off, "qbegin": qbegin, "qend": qend, "tbegin": tbegin, "tend": tend,
         "ops_off": a["ops_off"], "ops_len": a["ops_len"]}[k][0] = v
    return a
