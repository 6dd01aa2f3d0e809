"""The reverse-strand score entries (KERNELS.md 4n) measured, in one process on one GPU.  One JSON line per leg group.

--mode cost   what the flag costs calls that do not use it.  --other-lib PATH names libwfahip.so of the PARENT commit, built beforehand.
              Three legs alternate per step on the same inputs: the parent's entry on one context, the parent's entry on a second context
              (the yardstick of the yardstick: the difference between the two is what a difference means nothing below) and this tree's.
              Workloads: wfahip_score_batch_packed on 1e6 x 1 kbp @5 % (seed 3, 4/6/2, wf-adaptive 10/50/1), global (c3) and semi-global
              (g3); wfahip_score_matrix on 40 families x 50 variants of 1 kbp @5 % all against all (4e6 cells) at max_score 400, global
              and semi-global.  Status and score of the three legs are compared in every step.
--mode gain   what the feature buys: both strands of 1e6 x 1 kbp.  `flags`: every pair listed twice over ONE packed buffer, once flagged
              (wfahip_score_batch_packed_rc).  `materialised`: what a caller does without it -- reverse-complement every query on the
              host (numpy: a table look-up and a flip), wfahip_pack_pairs them, and score 2e6 pairs over the larger buffer with
              wfahip_score_batch_packed; its three parts are timed apart.  Wall ms per call, bytes uploaded (computed from the entries'
              upload rules), and the two legs' results compared; without a bound and, as a screen would run it, under --bound.

    python scripts/score_rc_bench.py --mode cost --other-lib parent/wfa_amd/lib/libwfahip.so [--pairs 1000000] [--steps 5]
    python scripts/score_rc_bench.py --mode gain [--pairs 1000000] [--steps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


class OtherLib:
    """wfahip_score_batch_packed and wfahip_score_matrix of another build of the library, through its C ABI"""

    def __init__(self, path, w, glob):
        from wfa_amd import _lib as L
        self.L, self.lib = L, C.CDLL(path)
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        self.lib.wfahip_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.lib.wfahip_destroy.argtypes = [vp]
        self.lib.wfahip_score_batch_packed.argtypes = [vp, C.POINTER(L.Params), vp, u64, vp, vp, vp, vp, u64, u32, C.POINTER(L.Scores)]
        self.lib.wfahip_score_matrix.argtypes = [vp, C.POINTER(L.Params), vp, u64, vp, vp, u64, vp, vp, u64, u32, vp, vp, u64]
        self.lib.wfahip_scores_free.argtypes = [C.POINTER(L.Scores)]
        self.lib.wfahip_last_timing.argtypes = [vp, C.POINTER(L.Timing)]
        self.ctx = vp()
        assert self.lib.wfahip_create(0, C.byref(self.ctx)) == 0
        self.prm = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert self.prm.AdaptiveReduction(w.DefaultAdaptiveOption) is None

    def score_packed(self, pk):
        packed, qw, ql, tw, tl = pk
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        out, prm = self.L.Scores(), self.prm._params()
        rc = self.lib.wfahip_score_batch_packed(self.ctx, C.byref(prm), vp(packed), packed.size, vp(qw), vp(ql), vp(tw), vp(tl), len(ql), 0, C.byref(out))
        assert rc == 0, rc
        n = int(out.n)
        st, sc = np.ctypeslib.as_array(out.status, shape=(n,)).copy(), np.ctypeslib.as_array(out.score, shape=(n,)).copy()
        self.lib.wfahip_scores_free(C.byref(out))
        return st, sc

    def score_matrix(self, blob, off, ln, bound):
        n = len(ln)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        st, sc, prm = np.zeros((n, n), np.int32), np.zeros((n, n), np.uint32), self.prm._params()
        rc = self.lib.wfahip_score_matrix(self.ctx, C.byref(prm), vp(blob), blob.size, vp(off), vp(ln), n, vp(off), vp(ln), n, bound, vp(st), vp(sc), n)
        assert rc == 0, rc
        return st, sc

    def last_timing(self):
        t = self.L.Timing()
        assert self.lib.wfahip_last_timing(self.ctx, C.byref(t)) == 0
        return t

    def close(self):
        self.lib.wfahip_destroy(self.ctx)


def run_legs(name, fns, steps, extra=None):
    """fns: (leg, call, who answers last_timing); a warm-up, then the legs alternate; every step's results must agree"""
    for _, fn, _ in fns:
        fn()
    legs = {leg: [] for leg, _, _ in fns}
    for _ in range(steps):
        res = {}
        for leg, fn, who in fns:
            t0 = time.perf_counter()
            res[leg] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            t = who.last_timing()
            legs[leg].append((dt, t.kernel_ms, t.main_kernel_kind, t.n_retried_pairs))
        first = res[fns[0][0]]
        for leg in legs:
            assert np.array_equal(res[leg][0], first[0]) and np.array_equal(res[leg][1], first[1]), (name, leg)
    out = {"workload": name, "steps": steps, **(extra or {})}
    for leg, v in legs.items():
        out[leg] = {"wall_ms": round(float(np.median([x[0] for x in v])), 2), "kernel_ms": round(float(np.median([x[1] for x in v])), 2),
                    "wall_ms_all": [round(x[0], 2) for x in v], "kernel_ms_all": [round(x[1], 2) for x in v], "kind": v[-1][2], "retried": v[-1][3]}
    out["results_equal"] = True
    print(json.dumps(out), flush=True)


def cost(args, w):
    from matrix_bench import families
    for name, glob in (("c3", True), ("g3", False)):
        arrays = w.generate_pairs(3, args.pairs, 1000, 0.05, n_threads=16)
        packed, qw, tw = w.pack_pairs(*arrays, n_threads=16)
        pk = (packed, qw, arrays[2], tw, arrays[4])
        al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
        pa, pb = OtherLib(args.other_lib, w, glob), OtherLib(args.other_lib, w, glob)
        run_legs("score_batch_packed " + name, [("parent_a", lambda: pa.score_packed(pk), pa), ("this", lambda: al.score_arrays_packed(*pk), al),
                                                ("parent_b", lambda: pb.score_packed(pk), pb)], args.steps, {"pairs": args.pairs})
        pa.close(), pb.close(), w.RecycleAligner(al)
    seqs = families(1, args.families, 50, 1000, 0.05)
    blob, off, ln, _, _ = w.make_blob(seqs, [b""] * len(seqs))
    for glob in (True, False):
        al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
        pa, pb = OtherLib(args.other_lib, w, glob), OtherLib(args.other_lib, w, glob)
        run_legs("score_matrix max_score 400 " + ("global" if glob else "semi-global"),
                 [("parent_a", lambda: pa.score_matrix(blob, off, ln, 400), pa), ("this", lambda: al.score_matrix_arrays(blob, off, ln, off, ln, max_score=400), al),
                  ("parent_b", lambda: pb.score_matrix(blob, off, ln, 400), pb)], args.steps, {"cells": len(seqs) ** 2})
        pa.close(), pb.close(), w.RecycleAligner(al)


COMP = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[a] = b


def host_revcomp(blob, q_off, q_len):
    """the queries of a batch reverse-complemented on the host: (blob of them, offsets)"""
    n, ln = len(q_len), int(q_len[0])
    if n > 1 and (q_len == ln).all() and (np.diff(q_off.astype(np.int64)) == int(q_off[1]) - int(q_off[0])).all():
        stride = int(q_off[1]) - int(q_off[0])
        rows = np.lib.stride_tricks.as_strided(blob[int(q_off[0]):], shape=(n, ln), strides=(stride, 1))
        return COMP[rows[:, ::-1]].reshape(-1), np.arange(n, dtype=np.uint64) * np.uint64(ln)
    parts = [COMP[blob[int(o):int(o) + int(k)][::-1]] for o, k in zip(q_off, q_len)]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(q_len[:-1], dtype=np.uint64)]).astype(np.uint64)


def gain(args, w):
    for name, glob in (("c3", True), ("g3", False)):
        blob, q_off, q_len, t_off, t_len = w.generate_pairs(3, args.pairs, 1000, 0.05, n_threads=16)
        n = args.pairs
        packed, qw, tw = w.pack_pairs(blob, q_off, q_len, t_off, t_len, n_threads=16)
        twice = lambda a: np.concatenate([a, a])
        flags = np.repeat(np.array([0, 1], np.uint8), n)
        al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
        pk2 = (packed, twice(qw), twice(q_len), twice(tw), twice(t_len))
        # the caller materialising it, timed part by part (each the median of three)
        t_rc, t_pack = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            rblob, roff = host_revcomp(blob, q_off, q_len)
            t_rc.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            zero = np.zeros(n, np.uint32)  # (the queries alone: a pair of each with an empty target, one pad word)
            rpacked, rqw, _ = w.pack_pairs(rblob, roff, q_len, np.zeros(n, np.uint64), zero, n_threads=16)
            big = np.concatenate([packed, rpacked])
            t_pack.append((time.perf_counter() - t0) * 1e3)
        mat = (big, np.concatenate([qw, rqw + np.uint64(packed.size)]), twice(q_len), twice(tw), twice(t_len))
        up = lambda words: 4 * int(words.size) + 24 * 2 * n
        for bound in (0, args.bound):  # (without a bound the wrong strand of every pair, an unrelated pair, runs to its end: kernels dominate)
            run_legs("both strands %s max_score %d" % (name, bound),
                     [("flags", lambda: al.score_arrays_packed_rc(*pk2, flags, max_score=bound), al),
                      ("materialised", lambda: al.score_arrays_packed(*mat, max_score=bound), al)], args.steps,
                     {"pairs": n, "host_revcomp_ms": round(float(np.median(t_rc)), 1), "pack_and_append_ms": round(float(np.median(t_pack)), 1),
                      "upload_bytes_flags": up(packed) + 2 * n, "upload_bytes_materialised": up(big)})
        w.RecycleAligner(al)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("cost", "gain"), required=True)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--families", type=int, default=40)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--bound", type=int, default=400, help="--mode gain: the max_score of its bounded legs")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("score_rc_bench: no GPU")
    import wfa_amd as w
    if args.mode == "cost":
        if not args.other_lib:
            raise SystemExit("--mode cost needs --other-lib")
        cost(args, w)
    else:
        gain(args, w)


if __name__ == "__main__":
    main()
