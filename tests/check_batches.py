"""The alignments the check's tests run over (tests/test_check_abi.py, tests/test_check_gpu.py): seeded batches, aligned once a
process by the CPU oracle on 8 threads and then left unchanged.  batch(name) gives dict(prm=(x, o, e, global), adaptive, seqs=(blob,
q_off, q_len, t_off, t_len), oracle=the oracle's BatchResult); packed(b) the same sequences as 2-bit words with every second query
flagged -- packed as its reverse complement, so that the strand the entries read is the one the results speak of."""
import functools

import numpy as np

from altext_pk_cases import pack_seq, revcomp

# name: (n_pairs, length, error rate, seed, (x, o, e, global), wf-adaptive or None, target overhangs)
SPEC = {
    "global 300":           (1500, 300, 0.05, 101, (4, 6, 2, 1), (10, 50, 1), False),
    "global 300, no adapt": (400, 300, 0.05, 102, (4, 6, 2, 1), None, False),
    "global 1k":            (500, 1000, 0.05, 103, (4, 6, 2, 1), (10, 50, 1), False),
    "global 1k, no adapt":  (100, 1000, 0.05, 104, (4, 6, 2, 1), None, False),
    "2/4/2":                (600, 300, 0.10, 105, (2, 4, 2, 1), (10, 50, 1), False),
    "semi-global 200":      (600, 200, 0.05, 106, (4, 6, 2, 0), (10, 50, 1), True),
    # short noisy pairs under an aggressive wf-adaptive.  The seed was searched for on the CPU, with the oracle, so that the batch
    # holds at least one pair each with M_DIFFERS, an _OVER flag and COST_UNDER (tests/test_check_abi.py asserts it)
    "aggressive":           (6000, 40, 0.20, 7, (4, 6, 2, 1), (4, 5, 1), False),
}
CLEAN = [k for k in SPEC if k != "aggressive"]


@functools.lru_cache(maxsize=None)
def batch(name):
    import wfa_amd
    from oracle import oracle as O
    n, length, err, seed, prm, adaptive, overhang = SPEC[name]
    seqs = wfa_amd.generate_pairs(seed=seed, n_pairs=n, length=length, error_rate=err)
    if overhang:
        rng = np.random.default_rng(seed)
        blob, q_off, q_len, t_off, t_len = seqs
        b = blob.tobytes()
        rnd = lambda k: bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))
        qs = [b[int(o):int(o) + int(k)] for o, k in zip(q_off, q_len)]
        ts = [rnd(int(rng.integers(1, 40))) + b[int(o):int(o) + int(k)] + rnd(int(rng.integers(1, 40))) for o, k in zip(t_off, t_len)]
        seqs = wfa_amd.make_blob(qs, ts)
    w = O.align_batch(O.make_params(*prm[:3], global_alignment=bool(prm[3]), adaptive=adaptive), *seqs, n_threads=8)
    for a in seqs:
        a.setflags(write=False)
    return dict(name=name, prm=prm, adaptive=adaptive, seqs=tuple(seqs), oracle=w)


def packed(b):
    """(words uint32, q_woff uint64, q_len uint32, t_woff uint64, t_len uint32, q_rc uint8) of a batch: pair i's target, then its
    query, every second query (odd i) flagged; the last sequence's pad word is the last word"""
    return _packed(b["name"])


@functools.lru_cache(maxsize=None)
def _packed(name):
    blob, q_off, q_len, t_off, t_len = batch(name)["seqs"]
    raw = blob.tobytes()
    n = len(q_len)
    q_rc = (np.arange(n) & 1).astype(np.uint8)
    q_woff, t_woff = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    parts, at = [], 0
    for i in range(n):
        q = raw[int(q_off[i]):int(q_off[i]) + int(q_len[i])]
        t = raw[int(t_off[i]):int(t_off[i]) + int(t_len[i])]
        for seq, off in ((t, t_woff), (revcomp(q) if q_rc[i] else q, q_woff)):
            w = pack_seq(seq)
            off[i] = at
            parts.append(w)
            at += len(w)
    out = (np.concatenate(parts), q_woff, np.array(q_len, np.uint32), t_woff, np.array(t_len, np.uint32), q_rc)
    for a in out:
        a.setflags(write=False)
    return out
