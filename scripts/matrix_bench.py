"""Score matrix against score batch: all against all of F families x k variants (1 kbp ancestors, 5 % divergence), global and
semi-global, wf-adaptive 10/50/1, max_score 0 and a bound.  wfahip_score_matrix runs against wfahip_score_batch on the
explicitly expanded pair list, alternating in one process, median of --reps after a warm-up; the two must agree cell for cell.
Prints cells/s, kernel ms, wall ms and the bytes each entry uploads, one JSON line per leg.

    python scripts/matrix_bench.py [--families 40] [--k 50] [--length 1000] [--rate 0.05] [--reps 5] [--bound 400]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("WFAHIP_DEBUG", "1")


def families(seed, n_fam, k, length, rate):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for _ in range(n_fam):
        anc = acgt[rng.integers(0, 4, length)]
        for _ in range(k):
            r = rng.random(length)
            sub = r < rate / 3
            dele = (r >= rate / 3) & (r < 2 * rate / 3)
            ins = (r >= 2 * rate / 3) & (r < rate)
            s = anc.copy()
            s[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
            parts = []
            for i in range(length):  # (insertions after the base, deletions drop it)
                if not dele[i]:
                    parts.append(s[i])
                if ins[i]:
                    parts.append(acgt[rng.integers(0, 4)])
            out.append(np.array(parts, np.uint8).tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=40)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--rate", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bound", type=int, default=400)
    a = ap.parse_args()
    import wfa_amd
    seqs = families(1, a.families, a.k, a.length, a.rate)
    n = len(seqs)
    blob, off, ln, _, _ = wfa_amd.make_blob(seqs, [b""] * n)
    # the expanded pair list of score_batch: (i, j) for every i, j, offsets into the same blob
    qi, tj = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    q_off, q_len, t_off, t_len = off[qi], ln[qi], off[tj], ln[tj]
    from wfa_amd import _lib
    packed_words = int(sum(_lib.lib().wfahip_packed_words(int(x)) for x in ln))
    up_matrix = 16 * n + 4 * packed_words
    up_batch = int(blob.size) + 24 * n * n
    for glob in (True, False):
        al = wfa_amd.New(wfa_amd.DefaultPenalties, wfa_amd.Options(GlobalAlignment=glob), device=0)
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(10, 50, 1)) is None
        for bound in (0, a.bound):
            runs = {"matrix": [], "batch": []}
            res = {}
            for rep in range(a.reps + 1):  # (rep 0: warm-up)
                for leg in ("matrix", "batch"):
                    t0 = time.perf_counter()
                    if leg == "matrix":
                        st, sc = al.score_matrix_arrays(blob, off, ln, off, ln, max_score=bound)
                    else:
                        st, sc = al.score_arrays(blob, q_off, q_len, t_off, t_len, max_score=bound)
                    wall = (time.perf_counter() - t0) * 1e3
                    t = al.last_timing()
                    res[leg] = (st.reshape(n, n), sc.reshape(n, n))
                    if rep:
                        runs[leg].append((wall, t.kernel_ms, t.main_kernel_kind, t.n_retried_pairs))
            agree = bool(np.array_equal(res["matrix"][0], res["batch"][0]) and np.array_equal(res["matrix"][1], res["batch"][1]))
            for leg in ("matrix", "batch"):
                wall = statistics.median(r[0] for r in runs[leg])
                kms = statistics.median(r[1] for r in runs[leg])
                print(json.dumps({"leg": leg, "global": glob, "max_score": bound, "n_seq": n, "cells": n * n,
                                  "cells_per_s": n * n / (wall / 1e3), "kernel_ms": round(kms, 2), "wall_ms": round(wall, 2),
                                  "bytes_uploaded": up_matrix if leg == "matrix" else up_batch, "kind": runs[leg][-1][2],
                                  "retried": runs[leg][-1][3], "agree": agree}), flush=True)
            if not agree:
                print("MISMATCH between the matrix and the batch entry", file=sys.stderr)
                return 1
        wfa_amd.RecycleAligner(al)
    return 0


if __name__ == "__main__":
    sys.exit(main())
