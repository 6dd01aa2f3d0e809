"""The reverse-strand alignment entry (KERNELS.md 4o) measured, in one process on one GPU.  One JSON line per workload.

--mode cost   what the flag costs calls that do not use it.  --other-lib PATH names libwfahip.so of the PARENT commit, built beforehand.
              Three legs alternate per step on the same inputs: the parent's wfahip_align_batch_packed on one context, the parent's on a
              second context (the yardstick of the yardstick: the spread between the two is what a difference means nothing below) and
              this tree's.  Workload: 1e6 x 1 kbp @5 % (seed 3, 4/6/2, wf-adaptive 10/50/1), global (c3) and semi-global (g3).  A
              warm-up, then the median of --steps; every field and CIGAR op of the three legs is compared in every step.
--mode gain   what the feature buys: both strands of 1e5 survivors of a screen.  `flags`: every pair listed twice over the ONE packed
              buffer, once flagged (wfahip_align_batch_packed_rc).  `materialised`: what a caller does without it -- wfahip_revcomp_packed
              on every query, the results appended to the buffer, new offset arrays, and wfahip_align_batch_packed over the larger
              buffer; the preparation is timed apart.  Wall ms per call, bytes uploaded (computed from the entry's upload rules), and
              the two legs' results compared.

    python scripts/align_rc_bench.py --mode cost --other-lib parent/wfa_amd/lib/libwfahip.so [--pairs 1000000] [--steps 5]
    python scripts/align_rc_bench.py --mode gain [--pairs 100000] [--steps 5]
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
FIELDS = ("status", "score", "tbegin", "tend", "qbegin", "qend", "align_len", "matches", "gaps", "gap_regions", "ops_len", "ops")


class OtherLib:
    """wfahip_align_batch_packed of another build of the library, through its C ABI"""

    def __init__(self, path, w, glob):
        from wfa_amd import _lib as L
        self.L, self.w, self.lib = L, w, C.CDLL(path)
        vp, u64 = C.c_void_p, C.c_uint64
        self.lib.wfahip_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.lib.wfahip_destroy.argtypes = [vp]
        self.lib.wfahip_align_batch_packed.argtypes = [vp, C.POINTER(L.Params), vp, u64, vp, vp, vp, vp, u64, C.POINTER(L.Results)]
        self.lib.wfahip_results_free.argtypes = [C.POINTER(L.Results)]
        self.lib.wfahip_last_timing.argtypes = [vp, C.POINTER(L.Timing)]
        self.ctx = vp()
        assert self.lib.wfahip_create(0, C.byref(self.ctx)) == 0
        self.prm = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert self.prm.AdaptiveReduction(w.DefaultAdaptiveOption) is None

    def align_packed(self, pk):
        packed, qw, ql, tw, tl = pk
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        out, prm = self.L.Results(), self.prm._params()
        rc = self.lib.wfahip_align_batch_packed(self.ctx, C.byref(prm), vp(packed), packed.size, vp(qw), vp(ql), vp(tw), vp(tl), len(ql), C.byref(out))
        assert rc == 0, rc
        try:
            return self.w.BatchResult.from_c(out, len(ql))
        finally:
            self.lib.wfahip_results_free(C.byref(out))  # (the library that made the arrays takes them back)

    def last_timing(self):
        t = self.L.Timing()
        assert self.lib.wfahip_last_timing(self.ctx, C.byref(t)) == 0
        return t

    def close(self):
        self.lib.wfahip_destroy(self.ctx)


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def run_legs(name, fns, steps, extra=None):
    """fns: (leg, call, who answers last_timing); a warm-up, then the legs alternate; every step's results must agree"""
    for _, fn, _ in fns:
        fn()
    legs = {leg: [] for leg, _, _ in fns}
    for _ in range(steps):
        first = None
        for leg, fn, who in fns:
            t0 = time.perf_counter()
            res = fn()
            dt = (time.perf_counter() - t0) * 1e3
            t = who.last_timing()
            legs[leg].append((dt, t.kernel_ms, t.main_kernel_kind, t.n_retried_pairs))
            if first is None:
                first = res
            else:
                assert same(res, first), (name, leg)
            del res
    out = {"workload": name, "steps": steps, **(extra or {})}
    for leg, v in legs.items():
        out[leg] = {"wall_ms": round(float(np.median([x[0] for x in v])), 2), "kernel_ms": round(float(np.median([x[1] for x in v])), 2),
                    "wall_ms_all": [round(x[0], 2) for x in v], "kernel_ms_all": [round(x[1], 2) for x in v], "kind": v[-1][2], "retried": v[-1][3]}
    out["results_equal"] = True
    print(json.dumps(out), flush=True)


def cost(args, w):
    for name, glob in (("c3", True), ("g3", False)):
        arrays = w.generate_pairs(3, args.pairs, 1000, 0.05, n_threads=16)
        packed, qw, tw = w.pack_pairs(*arrays, n_threads=16)
        pk = (packed, qw, arrays[2], tw, arrays[4])
        al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
        assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
        pa, pb = OtherLib(args.other_lib, w, glob), OtherLib(args.other_lib, w, glob)
        run_legs("align_batch_packed " + name, [("parent_a", lambda: pa.align_packed(pk), pa), ("this", lambda: al.align_arrays_packed(*pk), al),
                                                ("parent_b", lambda: pb.align_packed(pk), pb)], args.steps, {"pairs": args.pairs})
        pa.close(), pb.close(), w.RecycleAligner(al)


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
        # the caller materialising the reverse strand: revcomp_packed per query, appended behind the buffer, new offsets
        t0 = time.perf_counter()
        parts, rqw, pos = [packed], np.empty(n, np.uint64), packed.size
        for i in range(n):
            r = w.revcomp_packed(packed[int(qw[i]):], int(q_len[i]))
            rqw[i] = pos
            parts.append(r)
            pos += r.size
        big = np.concatenate(parts)
        mat = (big, np.concatenate([qw, rqw]), twice(q_len), twice(tw), twice(t_len))
        prep_ms = (time.perf_counter() - t0) * 1e3
        up = lambda words, rc: 4 * int(words.size) + 24 * 2 * n + (2 * n if rc else 0)
        run_legs("both strands " + name,
                 [("flags", lambda: al.align_arrays_packed_rc(*pk2, flags), al), ("materialised", lambda: al.align_arrays_packed(*mat), al)], args.steps,
                 {"pairs": n, "prepare_materialised_ms": round(prep_ms, 1), "upload_bytes_flags": up(packed, True), "upload_bytes_materialised": up(big, False)})
        w.RecycleAligner(al)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("cost", "gain"), required=True)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if args.pairs is None:
        args.pairs = 1_000_000 if args.mode == "cost" else 100_000
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("align_rc_bench: no GPU")
    import wfa_amd as w
    if args.mode == "cost":
        if not args.other_lib:
            raise SystemExit("--mode cost needs --other-lib")
        cost(args, w)
    else:
        gain(args, w)


if __name__ == "__main__":
    main()
