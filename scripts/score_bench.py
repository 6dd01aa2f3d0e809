"""Score-only against full alignment on the same host inputs, in one process (include/wfa_hip.h: wfahip_score_batch vs
wfahip_align_batch).  Workloads as bench.py generates them: c3 = 1e6 x 1 kbp @5 %, seed 3, global, wf-adaptive 10/50/1,
penalties 4/6/2; g3 = the same pairs semi-global.  After a warm-up of each entry, the two calls alternate --steps times;
per entry: pairs/s, wall ms per call (host clock around the synchronous call) and the kernel ms last_timing reports.
The scores of the two entries must agree.  One JSON line per workload.

Long-read legs (wfa_score_long_kernel, KERNELS.md 4i): L5 = 2e4 x 50 kbp @5 %, l5 = 500 x 50 kbp @5 %, global, 4/6/2,
wf-adaptive 10/50/1, seed 5; --pairs scales L5 down for a rehearsal.  --other-lib PATH adds a third leg: wfahip_score_batch of
ANOTHER build of the library (the parent commit's, built beforehand) on the same inputs, alternating with the two others in
the same process, so that the new score path is read against the old one and against that one's own run-to-run spread.

    python scripts/score_bench.py [--configs c3,g3] [--pairs 1000000] [--steps 5]
    python scripts/score_bench.py --configs L5,l5 [--other-lib parent/wfa_amd/lib/libwfahip.so]
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

# name: (global alignment, pairs, read length, error rate, seed); pairs None = --pairs
CONFIGS = {"c3": (True, None, 1000, 0.05, 3), "g3": (False, None, 1000, 0.05, 3),
           "L5": (True, 20000, 50000, 0.05, 5), "l5": (True, 500, 50000, 0.05, 5)}


class OtherLib:
    """wfahip_score_batch of another build of the library, through its C ABI (the entry's signature has not changed)."""

    def __init__(self, path, w, glob):
        from wfa_amd import _lib as L
        self.L, self.lib = L, C.CDLL(path)
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        self.lib.wfahip_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.lib.wfahip_destroy.argtypes = [vp]
        self.lib.wfahip_score_batch.argtypes = [vp, C.POINTER(L.Params), vp, u64, vp, vp, vp, vp, u64, u32, C.POINTER(L.Scores)]
        self.lib.wfahip_scores_free.argtypes = [C.POINTER(L.Scores)]
        self.lib.wfahip_last_timing.argtypes = [vp, C.POINTER(L.Timing)]
        self.ctx = vp()
        assert self.lib.wfahip_create(0, C.byref(self.ctx)) == 0
        self.prm = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert self.prm.AdaptiveReduction(w.DefaultAdaptiveOption) is None

    def score(self, arrays):
        blob, q_off, q_len, t_off, t_len = arrays
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        out, prm = self.L.Scores(), self.prm._params()
        rc = self.lib.wfahip_score_batch(self.ctx, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len), vp(t_off), vp(t_len), len(q_len), 0,
                                         C.byref(out))
        assert rc == 0, rc
        n = int(out.n)
        st = np.ctypeslib.as_array(out.status, shape=(n,)).copy()
        sc = np.ctypeslib.as_array(out.score, shape=(n,)).copy()
        self.lib.wfahip_scores_free(C.byref(out))
        return st, sc

    def last_timing(self):
        t = self.L.Timing()
        assert self.lib.wfahip_last_timing(self.ctx, C.byref(t)) == 0
        return t

    def close(self):
        self.lib.wfahip_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,g3")
    ap.add_argument("--pairs", type=int, default=None, help="pairs of c3 / g3 (default 1e6); scales L5 down when given")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--other-lib", default=None, help="libwfahip.so of another build: its wfahip_score_batch runs as a third leg")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU")
    import wfa_amd as w
    for name in args.configs.split(","):
        glob, pairs, length, err, seed = CONFIGS[name]
        if pairs is None:
            pairs = args.pairs or 1_000_000
        elif name == "L5" and args.pairs:
            pairs = args.pairs
        arrays = w.generate_pairs(seed, pairs, length, err, n_threads=16)
        al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
        fns = [("align", lambda: al.align_arrays(*arrays), al), ("score", lambda: al.score_arrays(*arrays), al)]
        other = None
        if args.other_lib:
            other = OtherLib(args.other_lib, w, glob)
            fns.append(("score_other", lambda: other.score(arrays), other))
        for _, fn, _ in fns:
            fn()  # warm-up: buffers, code objects
        legs = {leg: [] for leg, _, _ in fns}
        for _ in range(args.steps):
            res = {}
            for leg, fn, who in fns:
                t0 = time.perf_counter()
                res[leg] = fn()
                dt = (time.perf_counter() - t0) * 1e3
                t = who.last_timing()
                legs[leg].append((dt, t.kernel_ms, t.main_kernel_kind, t.n_retried_pairs, t.arena_bytes))
            ref = res["align"]
            want = np.where(ref.status == 0, ref.score, 0)
            for leg in legs:  # the scores are compared in every step
                if leg != "align":
                    st, sc = res[leg]
                    assert np.array_equal(st, ref.status) and np.array_equal(sc, want), (name, leg)
        out = {"config": name, "pairs": pairs, "steps": args.steps}
        for leg, v in legs.items():
            wall = float(np.median([x[0] for x in v]))
            out[leg] = {"pairs_per_s": pairs / wall * 1e3, "wall_ms": wall, "kernel_ms": float(np.median([x[1] for x in v])),
                        "main_kernel_kind": v[-1][2], "n_retried_pairs": v[-1][3], "arena_bytes": v[-1][4],
                        "wall_ms_all": [round(x[0], 2) for x in v], "wall_ms_spread": round(max(x[0] for x in v) - min(x[0] for x in v), 2)}
        out["scores_equal"] = True
        print(json.dumps(out), flush=True)
        if other:
            other.close()
        w.RecycleAligner(al)


if __name__ == "__main__":
    main()
