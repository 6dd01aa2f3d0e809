"""Synthetic records and ops for the CIGAR text entries (tests/test_cigar_abi.py on the host renderer, tests/test_cigar_gpu.py on the
kernels): no alignment is involved, the entries take any records.  A case is (status, [op words]); lay_out() scatters the cases' ops
through one op array out of pair order with unreferenced words between them, and render() is the Python restatement of the
reference's rule (AlignmentResult.CIGAR in wfa_amd/aligner.py)."""
import numpy as np

OK, EMPTY, TOO_LONG, NO_MEMORY, OVER_MAX = 0, 1, 2, 4, 8
# every count at which the number of digits changes, the largest u32, and 0
COUNTS = [0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000,
          999999999, 1000000000, 4294967295]
LETTERS = b"MDIXH~"  # the reference's five and one byte outside them: rendered verbatim
JUNK = 0x5A5A5A5A5A5A5A5A  # an unreferenced op word ('Z', count 1 515 870 810: ten digits if it were ever rendered)
STALE_OFF, STALE_LEN = (1 << 40) + 3, 77  # what the record of a failed pair may hold: far outside any op array


def op(letter, count):
    return ((letter if isinstance(letter, int) else ord(letter)) << 32) | count


def base_cases():
    c = []
    c.append((OK, [op(LETTERS[i % len(LETTERS)], n) for i, n in enumerate(COUNTS)]))          # digit boundaries, every letter
    c.append((OK, [op(LETTERS[(i + 3) % len(LETTERS)], n) for i, n in enumerate(reversed(COUNTS))]))
    c.append((OK, [op("M", n) for n in COUNTS]))
    c.append((OK, [op("X", 1)]))                                                              # no M: empty when trimmed (A against C)
    c.append((OK, [op("D", 3), op("I", 2), op("X", 1), op("H", 12)]))                         # no M, several ops
    c.append((OK, [op("M", 150)]))                                                            # a single op M
    c.append((OK, [op("M", 5), op("X", 1), op("I", 2), op("D", 3), op("H", 4)]))              # M only first
    c.append((OK, [op("I", 1), op("D", 2), op("X", 3), op("H", 1), op("M", 7)]))              # M only last
    c.append((OK, [op("I", 10), op("D", 2), op("X", 3), op("H", 100), op("M", 7), op("X", 1), op("M", 99), op("H", 1), op("X", 1),
                   op("D", 1000), op("I", 9)]))                                               # leading and trailing runs of I D X H
    c.append((OK, [op("M", 1), op("D", 1), op("I", 22), op("X", 333), op("H", 4444), op("~", 5), op("M", 2)]))  # two M, all between kept
    c.append((OK, [op("H", 2), op("M", 1), op("D", 1), op("M", 1), op("I", 1), op("M", 10), op("X", 7)]))       # three M
    c.append((OK, []))                                                                        # ops_len 0
    for st in (EMPTY, TOO_LONG, NO_MEMORY, OVER_MAX, 101):                                    # not OK: stale words, nothing rendered
        c.append((st, None))
    return c


def seam_cases(seed=5):
    """pairs of 0, 1, 63, 64, 65, 127, 128, 129 and 200 ops -- the seams of the write kernel's 64-op rounds -- with counts of one to
    four digits (so that the carry between rounds is not a multiple of anything); two pairs of 200 ops have their only M ops at 0 and
    199, and at 64 and 128"""
    rng = np.random.default_rng(seed)
    non_m = b"DIXH"

    def rand_ops(n, m_at=None):
        out = []
        for k in range(n):
            count = int(rng.choice([1, 7, 12, 345, 6789, 10, 100]))
            if m_at is None:
                letter = LETTERS[int(rng.integers(0, 5))]
            else:
                letter = ord("M") if k in m_at else non_m[int(rng.integers(0, 4))]
            out.append(op(letter, count))
        return out
    c = [(OK, rand_ops(n)) for n in (0, 1, 63, 64, 65, 127, 128, 129, 200)]
    c.append((OK, rand_ops(200, m_at=(0, 199))))
    c.append((OK, rand_ops(200, m_at=(64, 128))))
    c.append((OK, rand_ops(129, m_at=(63,))))
    c.append((OK, rand_ops(129, m_at=())))
    return c


def lay_out(cases, seed=1, junk=True):
    """(status int32, ops_off uint64, ops_len uint32, ops uint64): the cases' ops placed in a shuffled order, 0 to 5 junk words before
    each and a few behind the last; a case that is not OK gets stale ops_off / ops_len"""
    rng = np.random.default_rng(seed)
    n = len(cases)
    status = np.array([c[0] for c in cases], np.int32)
    ops_off, ops_len = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    words = []
    for i in rng.permutation(n):
        if junk:
            words += [JUNK] * int(rng.integers(0, 6))
        st, ops = cases[i]
        if st != OK:
            ops_off[i], ops_len[i] = STALE_OFF, STALE_LEN
            continue
        ops_off[i], ops_len[i] = len(words), len(ops)
        words += ops
    if junk:
        words += [JUNK] * 3
    return status, ops_off, ops_len, np.array(words, np.uint64)


def render(cases, only_aligned):
    """per case the bytes AlignmentResult.CIGAR(only_aligned) gives (b"" for a case that is not OK)"""
    import wfa_amd
    return [wfa_amd.AlignmentResult(Ops=list(ops)).CIGAR(bool(only_aligned)).encode("latin-1") if st == OK else b"" for st, ops in cases]


def expected(cases, only_aligned):
    """(text uint8, off uint64 [n + 1]) as the entries must return them"""
    parts = render(cases, only_aligned)
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64) if parts else 0
    return np.frombuffer(b"".join(parts), np.uint8), off


def records(status, ops_off, ops_len, seed=2):
    """device records int32-viewable uint32 [n, 16]: STATUS, OPS_LEN and OPS_OFF as given, every other word junk"""
    rng = np.random.default_rng(seed)
    n = len(status)
    rec = rng.integers(0, 1 << 32, size=(n, 16), dtype=np.uint64).astype(np.uint32)
    rec[:, 0] = status.astype(np.uint32)
    rec[:, 10] = ops_len
    rec[:, 11] = (ops_off & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rec[:, 12] = (ops_off >> np.uint64(32)).astype(np.uint32)
    return rec
