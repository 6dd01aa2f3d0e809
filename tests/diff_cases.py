"""The difference string (include/wfa_hip.h: wfahip_diff_text_device and its siblings; the rule is wfa_amd/csrc/wfa_diff.hpp's) restated
in Python over exact integers, sharing no code with the header: tests/test_diff_abi.py holds the host entries against it,
tests/test_diff_gpu.py and tests/test_diff_packed_gpu.py the kernels.  A case is altext_cases' (status, [op words], query bytes, target
bytes, qbegin, qend, tbegin, tend); cases() is that module's set and the seams that are this text's own; expected() is what the entries
must return; apply_diff() is the inverse a consumer would write -- the query's window from the target's window and the string."""
import re

import numpy as np

import altext_cases as A
from cigar_cases import OK, op  # noqa: F401

LANE_BYTES = 16   # wfa_diff.hpp's DIFF_LANE_BYTES: the write kernel renders an op of at most this many bytes in its own lane
LONG = 70001      # an op no lane may walk alone
_LC = bytes(b + 32 if 65 <= b <= 90 else b for b in range(256))


def lc(b):
    return bytes(b).translate(_LC)


def render(ops, q, t):
    """the text of a list of op words over the windows q and t; asserts that the ops stay inside them (a slice would truncate)"""
    out, qp, tp = [], 0, 0
    for o in ops:
        letter, n = int(o) >> 32, int(o) & 0xFFFFFFFF
        if letter in (ord("M"), ord("X")):
            assert qp + n <= len(q) and tp + n <= len(t)
            if n and letter == ord("M"):
                out.append(b":" + str(n).encode())
            elif n:
                tok = np.empty((n, 3), np.uint8)
                tok[:, 0] = ord("*")
                tok[:, 1] = np.frombuffer(lc(t[tp:tp + n]), np.uint8)
                tok[:, 2] = np.frombuffer(lc(q[qp:qp + n]), np.uint8)
                out.append(tok.tobytes())
            qp, tp = qp + n, tp + n
        elif letter == ord("I"):
            assert tp + n <= len(t)
            if n:
                out.append(b"-" + lc(t[tp:tp + n]))
            tp += n
        elif letter in (ord("D"), ord("H")):
            assert qp + n <= len(q)
            if n:
                out.append(b"+" + lc(q[qp:qp + n]))
            qp += n
    return b"".join(out)


def diff_of(case, only_aligned):
    """the difference string of a case (empty for a case that is not OK, without ops, or trimmed without an M op)"""
    st, ops, q, t, qbegin, qend, tbegin, tend = case
    if st != OK or not ops:
        return b""
    if not only_aligned:
        return render(ops, q, t)
    a, b = A.trim(ops)
    if b == 0:
        return b""
    assert 1 <= qbegin and qbegin - 1 <= qend <= len(q) and 1 <= tbegin and tbegin - 1 <= tend <= len(t)
    return render(ops[a:b], q[qbegin - 1:qend], t[tbegin - 1:tend])


def expected(cases_, only_aligned):
    """(text uint8, off uint64 [n + 1]) as the entries must return them, over the case tuples of cases() and of
    altext_pk_cases.with_acgt(cases()); a case object that occurs again is rendered once"""
    seen, parts = {}, []
    for c in cases_:
        if id(c) not in seen:
            seen[id(c)] = diff_of(c, only_aligned)
        parts.append(seen[id(c)])
    off = np.zeros(len(parts) + 1, np.uint64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return np.frombuffer(b"".join(parts), np.uint8), off


_TOKEN = re.compile(rb":([0-9]+)|\*(.)(.)|-([^:*+-]+)|\+([^:*+-]+)", re.S)


def apply_diff(target_window, text):
    """the query's window from the target's window and the string, for sequences over A C G T (the string spells bases in lower
    case; a consumer of upper-case sequences upper-cases them).  Asserts what the string says of the target, and that both are
    used up."""
    target_window, text = bytes(target_window), bytes(text)
    out, tp, at = [], 0, 0
    while at < len(text):
        m = _TOKEN.match(text, at)
        assert m is not None, f"no token at byte {at}"
        at = m.end()
        if m.group(1) is not None:
            n = int(m.group(1))
            assert tp + n <= len(target_window)
            out.append(target_window[tp:tp + n])
            tp += n
        elif m.group(2) is not None:
            assert lc(target_window[tp:tp + 1]) == m.group(2) != m.group(3)
            out.append(m.group(3).upper())
            tp += 1
        elif m.group(4) is not None:
            n = len(m.group(4))
            assert lc(target_window[tp:tp + n]) == m.group(4)
            tp += n
        else:
            out.append(m.group(5).upper())
    assert tp == len(target_window)
    return b"".join(out)


def match_counts(text):
    """the sum of the string's :n counts"""
    return sum(int(x) for x in re.findall(rb":([0-9]+)", bytes(text)))


def extra_cases(seed=19):
    """the seams that are the difference string's own"""
    rng = np.random.default_rng(seed)
    c = []
    # counts of 1, 2, 3 and 4 digits (ten digits need a gigabase: ten_digit_case())
    c.append(A.make([op("M", 7), op("X", 1), op("M", 42), op("I", 1), op("M", 123), op("D", 1), op("M", 1000)], rng))
    # an X run behind 2 .. 5 bytes of text: its 3-byte tokens cross every residue of a 4-byte group, in the sweep (7 columns) and in
    # the lane's own loop (2 and 5 columns)
    for r in range(4):
        c.append(A.make([op("D", r + 1), op("X", 7), op("M", 3), op("X", 2), op("I", r + 2), op("X", 5), op("M", 1)], rng, slack=r))
    # gaps of 15, 16 and 17 letters -- 16, 17 and 18 bytes, the seam of the lane-per-op bound -- of every gap letter; X ops of 5 and 6
    seam = []
    for k, letter in enumerate("IDHDHIHID"):
        seam += [op("M", 1 + k), op(letter, 15 + k // 3)]
    c.append(A.make(seam + [op("M", 2), op("X", 5), op("M", 1), op("X", 6), op("M", 3)], rng, slack=4))
    c.append(A.make([op("I", 16), op("D", 16), op("X", 6), op("H", 17), op("I", 15)], rng))          # no M op: long ops back to back
    # one op of 70 001 columns of each kind
    c.append(A.make([op("M", 1), op("X", LONG), op("M", 1)], rng))
    c.append(A.make([op("I", LONG), op("M", 2)], rng, slack=3))
    c.append(A.make([op("M", 1), op("H", LONG)], rng))
    c.append(A.make([op("M", LONG)], rng))
    # every byte value: upper case, lower case and everything else
    every, back = bytes(range(256)), bytes(range(255, -1, -1))
    c.append((OK, [op("X", 256)], every, back, 1, 256, 1, 256))
    c.append((OK, [op("M", 2), op("D", 124), op("I", 130), op("X", 3), op("H", 125), op("I", 119), op("M", 2)], every, back, 1, 256, 1, 256))
    c.append((OK, [op("D", 3), op("M", 1), op("X", 4), op("I", 9), op("M", 1)], b"AZaz@[`{09", b"MmNn\x00\xff\x7f\x80ZzAa~-+", 4, 9, 1, 15))
    return c


def cases(seed=7):
    return A.cases(seed) + extra_cases()


TEN_DIGITS = 1000000007  # an 'M' op of ten digits: the entries read no base of it, but its bases must lie inside the sequences


def ten_digit_case(target_letter, query_letter):
    """(ops, bases of each sequence, the text) of X 2, M TEN_DIGITS, I 3 over sequences of one repeated base each: the entries read no
    base of the M op, but its bases must lie inside the sequences -- which may be one zero-filled buffer, query and target aliased"""
    ops = [op("X", 2), op("M", TEN_DIGITS), op("I", 3)]
    t, q = lc(target_letter), lc(query_letter)
    return ops, TEN_DIGITS + 5, (b"*" + t + q) * 2 + b":%d" % TEN_DIGITS + b"-" + t * 3
