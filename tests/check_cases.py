"""The check's rule restated in Python, and synthetic records, ops and sequences for its entries (tests/test_check_abi.py on the host
entries, tests/test_check_gpu.py on the kernels).  restate() is written from the rule's text in include/wfa_hip.h -- exact Python
integers, one numpy compare per op -- and shares no code with wfa_amd/csrc/wfa_check.hpp.  A case is a dict: name, status, ops (op
words), q / t (ACGT bytes, the strand the ops speak of), rec (the record's fields), claims (the names of the flags it is built to
raise under PARAMS) and the switches ops_bad / q_bad / t_bad (an op range or a sequence that leaves its buffer)."""
import functools

import numpy as np

import cigar_cases as K
from cigar_cases import OK, op  # noqa: F401
from altext_pk_cases import pack_seq, packed_words, revcomp

NAMES = ("OPS_RANGE", "LETTER", "ZERO", "UNMERGED", "NO_M", "SEQ_RANGE", "Q_OVER", "Q_UNDER", "T_OVER", "T_UNDER", "M_DIFFERS", "X_EQUAL",
         "NO_ROWS", "NO_ROWS_TRIMMED", "COST_OVER", "COST_UNDER", "STAT_ALIGN_LEN", "STAT_MATCHES", "STAT_GAPS", "STAT_GAP_REGIONS")
BIT = {n: 1 << k for k, n in enumerate(NAMES)}
ALL = (1 << 20) - 1
NONE = 0xFFFFFFFF
M32 = 0xFFFFFFFF
CHECK_FAILED = 16
PARAMS = (4, 6, 2, 1)                                   # x, o, e, global: what the cases' claims hold under
HUGE = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1)          # every penalty the largest u32
FIELDS_U32 = ("score", "align_len", "matches", "gaps", "gap_regions")
FIELDS_I32 = ("qbegin", "qend", "tbegin", "tend")
_Q, _T = set(b"MXDH"), set(b"MXI")


def names_of(flags):
    return frozenset(n for n in NAMES if flags & BIT[n])


def split(ops):
    return [(int(o) >> 32, int(o) & M32) for o in ops]


def m_range(ops):
    m = [k for k, (l, _) in enumerate(split(ops)) if l == ord("M")]
    return (m[0], m[-1] + 1) if m else (0, 0)


def sums(ops):
    """(columns, query bases, target bases) the ops consume"""
    c = q = t = 0
    for l, n in split(ops):
        c += n if (l in _Q or l in _T) else 0
        q += n if l in _Q else 0
        t += n if l in _T else 0
    return c, q, t


def cost_of(ops, prm):
    x, o, e = prm[:3]
    return sum(x * n if l == ord("X") else o + e * n if l in b"IDH" else 0 for l, n in split(ops))


def stats_of(ops):
    """process() over the ops: (align_len, matches, gaps, gap_regions), u32 wrapping"""
    a, b = m_range(ops)
    if b == 0:
        a, b = 0, min(1, len(ops))
    part = split(ops)[a:b]
    return (sum(n for _, n in part) & M32, sum(n for l, n in part if l == ord("M")) & M32,
            sum(n for l, n in part if l in b"ID") & M32, sum(1 for l, _ in part if l in b"ID") & M32)


def restate_pair(status, rec, ops, q, t, q_len, t_len, prm, packed):
    """the eight words of one pair.  ops: its op words, None where they leave the op buffer; q / t: its sequences as arrays of bytes
    or codes, None where one of them leaves the blob or the words"""
    if status != OK:
        return [0] * 8
    if ops is None:
        return [BIT["OPS_RANGE"] | BIT["NO_ROWS"] | BIT["NO_ROWS_TRIMMED"]] + [0] * 7
    so = split(ops)
    f = 0
    if any(l not in b"MXIDH" for l, _ in so):
        f |= BIT["LETTER"]
    if any(n == 0 for _, n in so):
        f |= BIT["ZERO"]
    if any(so[k][0] == so[k - 1][0] for k in range(1, len(so))):
        f |= BIT["UNMERGED"]
    if not any(l == ord("M") for l, _ in so):
        f |= BIT["NO_M"]
    _, q_used, t_used = sums(ops)
    cost = cost_of(ops, prm)
    seq_ok = q is not None and t is not None
    n_bad, first = 0, None
    if not seq_ok:
        f |= BIT["SEQ_RANGE"]
    else:
        qi = ti = col = 0
        for l, n in so:
            if l in b"MX":
                v = max(0, min(n, q_len - qi, t_len - ti))
                if v:
                    differ = q[qi:qi + v] != t[ti:ti + v]
                    bad = np.flatnonzero(differ if l == ord("M") else ~differ)
                    if bad.size:
                        f |= BIT["M_DIFFERS"] if l == ord("M") else BIT["X_EQUAL"]
                        n_bad += int(bad.size)
                        if first is None:
                            first = col + int(bad[0])
            col += n if (l in _Q or l in _T) else 0
            qi += n if l in _Q else 0
            ti += n if l in _T else 0
    f |= BIT["Q_OVER"] if q_used > q_len else BIT["Q_UNDER"] if q_used < q_len else 0
    f |= BIT["T_OVER"] if t_used > t_len else BIT["T_UNDER"] if t_used < t_len else 0
    for trimmed in (False, True):
        part = ops[slice(*m_range(ops))] if trimmed else ops
        cols, qs, ts = sums(part)
        if len(part) == 0 or (packed and cols == 0):
            continue
        ok = seq_ok
        qn, tn = q_len, t_len
        if ok and trimmed:
            for begin, end, ln in ((rec["qbegin"], rec["qend"], q_len), (rec["tbegin"], rec["tend"], t_len)):
                ok = ok and begin >= 1 and begin - 1 <= end <= ln
            qn, tn = rec["qend"] - rec["qbegin"] + 1, rec["tend"] - rec["tbegin"] + 1
        if not ok or qs > qn or ts > tn:
            f |= BIT["NO_ROWS_TRIMMED"] if trimmed else BIT["NO_ROWS"]
    if prm[3]:
        f |= BIT["COST_OVER"] if cost > rec["score"] else BIT["COST_UNDER"] if cost < rec["score"] else 0
    for name, v in zip(("align_len", "matches", "gaps", "gap_regions"), stats_of(ops)):
        if v != rec[name]:
            f |= BIT["STAT_" + name.upper()]
    return [f, min(cost, M32), min(q_used, M32), min(t_used, M32), min(n_bad, M32), NONE if first is None else min(first, NONE - 1), 0, 0]


def unpack_codes(words, woff, ln, rc):
    """the 2-bit codes of the ln bases packed at word woff, reverse-complemented if rc"""
    w = words[woff:woff + (ln + 15) // 16].astype(np.uint64)
    codes = ((w[:, None] >> (2 * np.arange(16, dtype=np.uint64))) & np.uint64(3)).reshape(-1)[:ln].astype(np.uint8)
    return (codes[::-1] ^ 2) if rc else codes


def restate(a, prm, packed=False, n_words=None, blob_bytes=None):
    """chk uint32 [n, 8] for arrays as arrays() returns them (or the same keys filled from real results)"""
    n = len(a["status"])
    out = np.zeros((n, 8), np.uint32)
    ops_all, cap = a["ops"], len(a["ops"])
    seqs, q_off, q_len, t_off, t_len = a["seqs"][:5]
    q_rc = a["seqs"][5] if packed else None
    size = (n_words if packed else blob_bytes)
    size = len(seqs) if size is None else size
    for i in range(n):
        st = int(a["status"][i])
        if st != OK:
            continue
        rec = {k: int(a[k][i]) for k in FIELDS_U32 + FIELDS_I32}
        L, off = int(a["ops_len"][i]), int(a["ops_off"][i])
        ops = None if (L > cap or off > cap - L) else [int(v) for v in ops_all[off:off + L]]
        ql, tl, qo, to = int(q_len[i]), int(t_len[i]), int(q_off[i]), int(t_off[i])
        q = t = None
        if ops is not None:
            if packed:
                if all(o <= size and packed_words(l) <= size - o for o, l in ((qo, ql), (to, tl))):
                    q, t = unpack_codes(seqs, qo, ql, q_rc is not None and bool(q_rc[i])), unpack_codes(seqs, to, tl, False)
            elif all(o <= size and l <= size - o for o, l in ((qo, ql), (to, tl))):
                q, t = seqs[qo:qo + ql], seqs[to:to + tl]
        out[i] = restate_pair(st, rec, ops, q, t, ql, tl, prm, packed)
    return out


def passed_of(status, chk, mask):
    """the pass array and the count the entries give for these words"""
    flagged = (np.asarray(status) == OK) & ((chk[:, 0] & np.uint32(mask)) != 0)
    return np.where(np.asarray(status) != OK, status, np.where(flagged, CHECK_FAILED, OK)).astype(np.int32), int(flagged.sum())


# ---- the synthetic set

def clean(name, ops, rng, claims=(), prm=PARAMS):
    """a case whose sequences, record and score agree with its ops under prm: M columns equal, X columns different"""
    q, t = bytearray(), bytearray()
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for l, n in split(ops):
        n = min(n, 1 << 17)  # (a count beyond that is a case that overruns on purpose)
        code = rng.integers(0, 4, n)
        b, o = acgt[code].tobytes(), acgt[(code + rng.integers(1, 4, n)) % 4].tobytes()
        if l == ord("M"):
            q += b
            t += b
        elif l == ord("X"):
            q += b
            t += o
        elif l == ord("I"):
            t += b
        elif l in b"DH":
            q += b
    a, b = m_range(ops)
    _, pq, pt = sums(ops[:a])
    _, wq, wt = sums(ops[a:b])
    st = stats_of(ops)
    i32 = lambda v: ((v + (1 << 31)) & M32) - (1 << 31)  # (a window of a case with huge counts wraps, as a record's word would)
    rec = dict(score=min(cost_of(ops, prm), M32), align_len=st[0], matches=st[1], gaps=st[2], gap_regions=st[3],
               qbegin=i32(pq + 1), qend=i32(pq + wq), tbegin=i32(pt + 1), tend=i32(pt + wt))
    return dict(name=name, status=OK, ops=list(ops), q=bytes(q), t=bytes(t), rec=rec, claims=frozenset(claims), ops_bad=False, q_bad=False,
                t_bad=False)


def changed(case, name, claims, **kw):
    """a copy of a case with fields of the record (score=.., qbegin=..), q / t / ops or a switch replaced"""
    c = dict(case, name=name, claims=frozenset(claims), rec=dict(case["rec"]))
    for k, v in kw.items():
        if k in c["rec"]:
            c["rec"][k] = v
        else:
            c[k] = v
    return c


def flip(seq, at, rng=None):
    b = bytearray(seq)
    b[at] = b"ACGT"[(b"ACGT".index(b[at]) + 1) % 4]
    return bytes(b)


BASE_OPS = [op("H", 2), op("I", 3), op("M", 9), op("X", 2), op("M", 30), op("D", 4), op("M", 7), op("I", 1), op("M", 5), op("X", 1), op("D", 2)]
N_OPS = [0, 1, 63, 64, 65, 128, 129, 200]


def rand_ops(n, rng, lo=1, hi=9):
    """n ops, neighbours of different letters, an M among the first and the last three"""
    out, prev = [], None
    for k in range(n):
        l = "M" if (k in (1, n - 2) or n == 1) else "MXIDH"[int(rng.integers(0, 5))]
        while l == prev:
            l = "MXIDH"[int(rng.integers(0, 5))]
        out.append(op(l, int(rng.integers(lo, hi))))
        prev = l
    return out


@functools.lru_cache(maxsize=None)
def cases(seed=23):
    """the set, as a tuple (built once a process; nothing changes a case)"""
    return tuple(_cases(seed))


def _cases(seed):
    rng = np.random.default_rng(seed)
    c = []
    base = clean("clean", BASE_OPS, rng)
    r = base["rec"]
    c.append(base)
    # ---- every flag alone, or with what the rule makes of it by itself
    c.append(changed(base, "ops range", ["OPS_RANGE", "NO_ROWS", "NO_ROWS_TRIMMED"], ops_bad=True))
    c.append(clean("letter", BASE_OPS[:4] + [op("~", 3)] + BASE_OPS[4:], rng, ["LETTER"]))
    c.append(clean("zero", BASE_OPS[:5] + [op("X", 0)] + BASE_OPS[5:], rng, ["ZERO"]))
    c.append(clean("unmerged", [op("M", 5), op("M", 3), op("X", 1), op("M", 2)], rng, ["UNMERGED"]))
    c.append(clean("no M", [op("X", 2), op("I", 1), op("D", 1)], rng, ["NO_M"]))
    c.append(clean("empty", [], rng, ["NO_M"]))
    c.append(changed(base, "q range", ["SEQ_RANGE", "NO_ROWS", "NO_ROWS_TRIMMED"], q_bad=True))
    c.append(changed(base, "t range", ["SEQ_RANGE", "NO_ROWS", "NO_ROWS_TRIMMED"], t_bad=True))
    c.append(changed(base, "q over", ["Q_OVER", "NO_ROWS"], q=base["q"][:-1]))           # the last op, a D behind the last M, overruns
    c.append(changed(base, "q under", ["Q_UNDER"], q=base["q"] + b"A"))
    c.append(changed(base, "t over", ["T_OVER", "NO_ROWS"], t=base["t"][:-1]))          # the X behind the last M overruns
    c.append(changed(base, "t under", ["T_UNDER"], t=base["t"] + b"C"))
    c.append(changed(base, "m differs", ["M_DIFFERS"], q=flip(base["q"], 2 + 4)))        # column 9 of the rows
    c.append(changed(base, "x equal", ["X_EQUAL"], t=base["t"][:12] + base["q"][11:12] + base["t"][13:]))  # column 14: q[11] against t[12]
    c.append(changed(base, "no rows trimmed", ["NO_ROWS_TRIMMED"], qbegin=0))
    c.append(changed(base, "cost over", ["COST_OVER"], score=r["score"] - 2))
    c.append(changed(base, "cost under", ["COST_UNDER"], score=r["score"] + 2))
    c.append(changed(base, "stat len", ["STAT_ALIGN_LEN"], align_len=r["align_len"] + 1))
    c.append(changed(base, "stat matches", ["STAT_MATCHES"], matches=r["matches"] - 1))
    c.append(changed(base, "stat gaps", ["STAT_GAPS"], gaps=r["gaps"] + 1))
    c.append(changed(base, "stat regions", ["STAT_GAP_REGIONS"], gap_regions=0))
    # ---- neighbouring steps together
    for st in (K.EMPTY, K.TOO_LONG, K.NO_MEMORY, K.OVER_MAX, 101):                       # 1 over 2, 5: stale words, offsets out of range
        c.append(changed(base, f"status {st}", [], status=st, ops_bad=True, q_bad=True, t_bad=True, score=77))
    c.append(changed(base, "ops range over all", ["OPS_RANGE", "NO_ROWS", "NO_ROWS_TRIMMED"], ops_bad=True, q_bad=True, score=1, matches=0,
                     q=base["q"][:3]))                                                   # 2 over 3 .. 10
    c.append(clean("letter zero unmerged", [op("M", 4), op("~", 0), op("~", 2), op("X", 1), op("I", 0), op("M", 1)], rng,
                   ["LETTER", "ZERO", "UNMERGED"]))                                      # 3 with 4: the cost and the sums go on
    c.append(clean("zero M only", [op("X", 3), op("M", 0), op("D", 1)], rng, ["ZERO"]))   # an M op of no column is an M op
    c.append(changed(base, "range, over, cost", ["SEQ_RANGE", "Q_OVER", "NO_ROWS", "NO_ROWS_TRIMMED", "COST_OVER", "STAT_GAPS"], q_bad=True,
                     q=flip(base["q"], 6)[:-2], score=0, gaps=0))                        # 5 stops 7, not 4, 6, 9, 10
    over = clean("m runs over both", [op("M", 40)], rng)
    c.append(changed(over, "m over, differs inside", ["Q_OVER", "T_OVER", "M_DIFFERS", "NO_ROWS", "NO_ROWS_TRIMMED"],
                     q=flip(over["q"], 37)[:38], t=over["t"][:39]))                      # 6 with 7: columns 38, 39 are not compared
    c.append(changed(over, "m over, clean inside", ["Q_OVER", "NO_ROWS", "NO_ROWS_TRIMMED"], q=over["q"][:38]))
    xo = clean("x over", [op("M", 3), op("X", 5)], rng)
    c.append(changed(xo, "x over by two", ["T_OVER", "NO_ROWS", "NO_ROWS_TRIMMED"], t=xo["t"][:-2], tend=7))  # TEND lies behind the target as well
    both = clean("both", BASE_OPS, rng)
    q2 = flip(flip(flip(both["q"], 2), 20), 54)                                          # columns 5, 23 and the last M column but one
    t2 = both["t"][:13] + both["q"][12:13] + both["t"][14:]                              # the second X column: q[12] against t[13]
    c.append(changed(both, "m differs and x equal", ["M_DIFFERS", "X_EQUAL"], q=q2, t=t2))
    c.append(changed(both, "bad columns and trimmed window", ["M_DIFFERS", "NO_ROWS_TRIMMED"], q=flip(both["q"], 2), tend=10 ** 6))  # 7 with 8
    c.append(changed(base, "rows, cost, stat", ["T_OVER", "NO_ROWS", "NO_ROWS_TRIMMED", "COST_UNDER", "STAT_GAP_REGIONS"], t=base["t"][:-3],
                     score=r["score"] + 1, gap_regions=r["gap_regions"] + 7))            # 8, 9, 10
    c.append(clean("no M, op 0 alone", [op("D", 7), op("I", 2), op("X", 1)], rng, ["NO_M"]))  # 10: align_len 7, gaps 7, one region
    # ---- counts of 0 and of 0xFFFFFFFF (under HUGE the cost does not fit 64 bits; under PARAMS it does not fit 32)
    huge = clean("huge counts", [op("M", 3), op("D", M32), op("X", M32), op("I", M32), op("M", 2)], rng)
    c.append(changed(huge, "huge counts", ["Q_OVER", "T_OVER", "NO_ROWS", "NO_ROWS_TRIMMED", "COST_OVER"], q=huge["q"][:40], t=huge["t"][:40]))
    hx = clean("huge x", [op("M", 2), op("X", M32)], rng)
    c.append(changed(hx, "huge x", ["Q_OVER", "T_OVER", "NO_ROWS", "COST_OVER", "X_EQUAL"], q=hx["q"][:10],
                     t=hx["t"][:9] + hx["q"][9:10]))                                     # eight X columns are compared, the last one equal
    c.append(clean("zeros", [op("I", 0), op("M", 0), op("X", 0)], rng, ["ZERO"]))
    # ---- shapes: the seams of the 64-op rounds, one long op, every length mod 16
    for n in N_OPS[1:]:
        c.append(clean(f"{n} ops", rand_ops(n, rng), rng))
    c.append(clean("70000 columns", [op("X", 1), op("M", 70001), op("I", 3)], rng))
    for n in range(16, 32):
        c.append(clean(f"len {n}", [op("M", n - 3), op("X", 1), op("M", 2)], rng))
    return c


def layout(cs, packed=False, flags=None, seed=5, junk_tails=None):
    """the sequences of the cases in one blob (bytes: the k-th at an offset of residue k mod 16, junk between them) or one word array
    (a flagged query packed as its reverse complement; junk_tails: a seed for random tail bits and pad words); the last one ends
    on the last byte / word.  A q_bad / t_bad sequence starts where its end leaves the buffer by one.  Returns (seqs, q_off, q_len,
    t_off, t_len[, q_rc])."""
    rng = np.random.default_rng(seed)
    tails = None if junk_tails is None else np.random.default_rng(junk_tails)
    n = len(cs)
    q_off, t_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    q_len, t_len = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    q_rc = np.array([1 if f else 0 for f in (flags if flags is not None else [0] * n)], np.uint8)
    parts, at, placed = [], 0, 0
    for i in rng.permutation(n):
        for seq, off, ln, is_q in ((cs[i]["t"], t_off, t_len, False), (cs[i]["q"], q_off, q_len, True)):
            if packed:
                pad = int(rng.integers(0, 3))
                parts.append(rng.integers(0, 1 << 32, pad, dtype=np.uint64).astype(np.uint32))
                piece = pack_seq(revcomp(seq) if (is_q and q_rc[i]) else seq, tails)
            else:
                pad = (placed % 16 - at) % 16 + 16 * int(rng.integers(0, 2))
                parts.append(rng.integers(0, 256, pad, dtype=np.uint8))
                piece = np.frombuffer(seq, np.uint8)
            at += pad
            off[i], ln[i] = at, len(seq)
            parts.append(piece)
            at += len(piece)
            placed += 1
    seqs = np.concatenate(parts).astype(np.uint32 if packed else np.uint8) if parts else np.zeros(0, np.uint32 if packed else np.uint8)
    for i, c in enumerate(cs):
        for bad, off, ln in ((c["q_bad"], q_off, q_len), (c["t_bad"], t_off, t_len)):
            if bad:
                need = packed_words(int(ln[i])) if packed else int(ln[i])
                off[i] = len(seqs) - need + 1
    return (seqs, q_off, q_len, t_off, t_len, q_rc) if packed else (seqs, q_off, q_len, t_off, t_len)


def arrays(cs, packed=False, flags=None, seed=11, junk_tails=None):
    """everything the entries take for a list of cases, as numpy arrays: the fields of a wfahip_results, the device records of the
    same contents (every other word junk), and the sequences"""
    status, ops_off, ops_len, ops = K.lay_out([(c["status"], c["ops"]) for c in cs], seed=seed)
    for i, c in enumerate(cs):
        if c["ops_bad"]:
            ops_off[i], ops_len[i] = len(ops) - len(c["ops"]) + 1, len(c["ops"])
    a = dict(status=status, ops_off=ops_off, ops_len=ops_len, ops=ops)
    for k in FIELDS_U32:
        a[k] = np.array([c["rec"][k] for c in cs], np.uint32)
    for k in FIELDS_I32:
        a[k] = np.array([c["rec"][k] for c in cs], np.int32)
    rec = K.records(status, ops_off, ops_len)
    rec[:, 1] = a["score"]
    rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5] = (a[k].view(np.uint32) for k in ("tbegin", "tend", "qbegin", "qend"))
    rec[:, 6], rec[:, 7], rec[:, 8], rec[:, 9] = a["align_len"], a["matches"], a["gaps"], a["gap_regions"]
    a["rec"] = rec
    a["seqs"] = layout(cs, packed, flags, seed=seed + 1, junk_tails=junk_tails)
    return a


def from_results(br, seqs):
    """restate()'s and the host entries' view of real results: a BatchResult (wfa_amd's or the oracle's) and the sequences' tuple"""
    a = {k: np.asarray(getattr(br, k)) for k in ("status", "ops_off", "ops_len", "ops") + FIELDS_U32 + FIELDS_I32}
    a["seqs"] = seqs
    return a
