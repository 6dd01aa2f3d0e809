"""Semi-global batches of mixed read lengths: the length-class routing of align_device (KERNELS.md 4m) against single-class sizing
and, with --other-lib, against another build of the library (the parent commit's, built beforehand) on the same inputs, the legs
alternating per step in one process.  One JSON line per workload; per leg pairs/s, wall ms per call (host clock around the
synchronous call, median and every value), the milliseconds of the wide launches (main_kernel_ms, summed over the classes; the
launches one by one on stderr with WFAHIP_DEBUG_TIMING=1), main_kernel_kind, the pairs on either side and arena_bytes.  The records'
status and score of all legs are compared in every step, outside the timed region.

Workloads (penalties 4/6/2, wf-adaptive 10/50/1, 5 % error):
    mix    --pairs semi-global pairs (default 1e6): 90 % of 150 bases, 9.9 % of 1 000, 0.1 % of 3 000, shuffled
    u300   --pairs / 10 semi-global pairs of 300 bases: a uniform batch, which must run as it did before there were classes
    pk     --pairs semi-global pairs of 1 000 bases through wfahip_align_batch (autopack) and wfahip_align_batch_packed
Legs: `host` = wfahip_align_batch, `device` = wfahip_align_batch_device on the batch resident in HBM; `*_one` = the same with
"wide_classes" 0; `*_other` = the other build; pk: `host`, `packed` (+ `_other`).

    python scripts/mixed_bench.py [--workloads mix,u300,pk] [--pairs 1000000] [--steps 3] [--other-lib parent/wfa_amd/lib/libwfahip.so]
        [--opt wide_bin_min_pairs=4096]
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
os.environ.setdefault("WFAHIP_DEBUG", "1")  # ("wide_classes", "wide_bin_min_pairs" are debug keys: refused without it)


def mixed_pairs(w, n, parts, seed):
    """parts: ((share, length), ..) -> one batch of n pairs, shuffled: the parts' blobs one after the other, the pair order permuted"""
    blobs, qo, ql, to, tl, base, left = [], [], [], [], [], 0, n
    for j, (share, length) in enumerate(parts):
        k = left if j == len(parts) - 1 else int(round(n * share))
        left -= k
        blob, q_off, q_len, t_off, t_len = w.generate_pairs(seed + j, k, length, 0.05, n_threads=16)
        qo.append(q_off + np.uint64(base)), to.append(t_off + np.uint64(base)), ql.append(q_len), tl.append(t_len)
        blobs += [blob, np.zeros(-len(blob) % 16, dtype=np.uint8)]
        base += len(blob) + (-len(blob) % 16)
    order = np.random.default_rng(seed).permutation(n)
    blob, q_off, q_len, t_off, t_len = (np.concatenate(x) for x in (blobs, qo, ql, to, tl))
    return blob, q_off[order].copy(), q_len[order].copy(), t_off[order].copy(), t_len[order].copy()


class Lib:
    """An aligner of this build (lib = None) or of another build through its C ABI (no alignment entry has changed its signature)."""

    def __init__(self, w, path=None, opts=()):
        from wfa_amd import _lib as L
        self.L, self.al = L, w.New(w.DefaultPenalties, w.Options(GlobalAlignment=False), device=0)
        assert self.al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
        self.lib, self.ctx = L.lib(), self.al._ctx
        if path:
            vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
            self.lib = C.CDLL(path)
            self.lib.wfahip_create.argtypes = [C.c_int, C.POINTER(vp)]
            self.lib.wfahip_destroy.argtypes = [vp]
            self.lib.wfahip_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
            self.lib.wfahip_align_batch.argtypes = [vp, C.POINTER(L.Params), vp, u64, vp, vp, vp, vp, u64, C.POINTER(L.Results)]
            self.lib.wfahip_align_batch_packed.argtypes = [vp, C.POINTER(L.Params), vp, u64, vp, vp, vp, vp, u64, C.POINTER(L.Results)]
            self.lib.wfahip_align_batch_device.argtypes = [vp, C.POINTER(L.Params), vp, u64, vp, vp, vp, vp, u64, u32, vp, vp, u64, C.POINTER(u64), vp]
            self.lib.wfahip_results_free.argtypes = [C.POINTER(L.Results)]
            self.lib.wfahip_last_timing.argtypes = [vp, C.POINTER(L.Timing)]
            self.ctx = vp()
            assert self.lib.wfahip_create(0, C.byref(self.ctx)) == 0
        self.own = bool(path)
        for kv in opts:
            k, v = kv.split("=")
            assert self.lib.wfahip_set_option(self.ctx, k.encode(), int(v)) == 0, kv

    def host(self, arrays, packed=False):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        a, res, prm = arrays, self.L.Results(), self.al._params()
        fn = self.lib.wfahip_align_batch_packed if packed else self.lib.wfahip_align_batch
        rc = fn(self.ctx, C.byref(prm), vp(a[0]), a[0].size, vp(a[1]), vp(a[2]), vp(a[3]), vp(a[4]), len(a[2]), C.byref(res))
        assert rc == 0, rc
        n = int(res.n)
        out = (np.ctypeslib.as_array(res.status, shape=(n,)).copy(), np.ctypeslib.as_array(res.score, shape=(n,)).copy())
        self.lib.wfahip_results_free(C.byref(res))
        return out

    def device(self, d, blob_bytes, n, max_len, d_rec, d_ops, ops_cap):
        needed, prm = C.c_uint64(), self.al._params()
        rc = self.lib.wfahip_align_batch_device(self.ctx, C.byref(prm), d[0].data_ptr(), blob_bytes, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                d[4].data_ptr(), n, max_len, d_rec.data_ptr(), d_ops.data_ptr(), ops_cap, C.byref(needed), None)
        assert rc == 0, rc

        def fetch():
            rec = d_rec[:, :2].cpu().numpy().view(np.uint32)
            st = rec[:, self.L.REC_STATUS].view(np.int32).copy()
            return st, np.where(st == 0, rec[:, self.L.REC_SCORE], 0).astype(np.uint32)
        return fetch

    def last_timing(self):
        t = self.L.Timing()
        assert self.lib.wfahip_last_timing(self.ctx, C.byref(t)) == 0
        return t

    def close(self):
        if self.own:
            self.lib.wfahip_destroy(self.ctx)
        self.al.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="mix,u300,pk")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--other-lib", default=None, help="libwfahip.so of another build: its entries run as further legs")
    ap.add_argument("--opt", action="append", default=[], help="library option key=value for this build's legs")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mixed_bench: no GPU")
    import wfa_amd as w
    from wfa_amd import _lib as L
    dev = torch.device("cuda", 0)
    for name in args.workloads.split(","):
        if name == "mix":
            n, arrays = args.pairs, mixed_pairs(w, args.pairs, ((0.9, 150), (0.099, 1000), (0.001, 3000)), 31)
        elif name == "u300":
            n = max(1, args.pairs // 10)
            arrays = w.generate_pairs(32, n, 300, 0.05, n_threads=16)
        else:
            n, arrays = args.pairs, w.generate_pairs(3, args.pairs, 1000, 0.05, n_threads=16)
        libs = {"": Lib(w, opts=args.opt)}
        if name != "pk":
            libs["_one"] = Lib(w, opts=args.opt + ["wide_classes=0"])
        if args.other_lib:
            libs["_other"] = Lib(w, args.other_lib)
        fns = []
        if name == "pk":
            pk = w.pack_pairs(*arrays, n_threads=16)
            pk = (pk[0], pk[1], arrays[2], pk[2], arrays[4])
            for sfx, lb in libs.items():
                fns.append(("host" + sfx, lambda lb=lb: lb.host(arrays), lb))
                fns.append(("packed" + sfx, lambda lb=lb: lb.host(pk, packed=True), lb))
        else:
            d = [torch.from_numpy(a).to(dev) for a in (arrays[0], arrays[1].view(np.int64), arrays[2].view(np.int32), arrays[3].view(np.int64),
                                                       arrays[4].view(np.int32))]
            max_len = int(max(arrays[2].max(), arrays[4].max()))
            ops_cap = int(arrays[2].astype(np.int64).sum() + arrays[4].astype(np.int64).sum()) + 2 * n + 1024
            d_rec = torch.zeros((n, L.REC_WORDS), dtype=torch.int32, device=dev)
            d_ops = torch.zeros(ops_cap, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            for sfx, lb in libs.items():
                fns.append(("host" + sfx, lambda lb=lb: lb.host(arrays), lb))
                fns.append(("device" + sfx, lambda lb=lb: lb.device(d, arrays[0].size, n, max_len, d_rec, d_ops, ops_cap), lb))
        for _, fn, _ in fns:
            fn()  # warm-up: buffers, code objects
        legs = {leg: [] for leg, _, _ in fns}
        for _ in range(args.steps):
            ref = None
            for leg, fn, who in fns:
                t0 = time.perf_counter()
                res = fn()
                dt = (time.perf_counter() - t0) * 1e3
                t = who.last_timing()
                legs[leg].append((dt, t.kernel_ms, t.main_kernel_ms, t.main_kernel_kind, t.n_packed_pairs, t.n_retried_pairs, t.arena_bytes, t.n_main_launches))
                st, sc = res() if callable(res) else res
                if ref is None:
                    ref = (st, sc)
                assert np.array_equal(st, ref[0]) and np.array_equal(sc, ref[1]), (name, leg)
        out = {"workload": name, "pairs": n, "steps": args.steps, "opts": args.opt}
        for leg, v in legs.items():
            wall = float(np.median([x[0] for x in v]))
            out[leg] = {"pairs_per_s": round(n / wall * 1e3), "wall_ms": round(wall, 2), "wall_ms_all": [round(x[0], 2) for x in v],
                        "kernel_ms": round(float(np.median([x[1] for x in v])), 2), "main_kernel_ms": round(float(np.median([x[2] for x in v])), 2),
                        "main_kernel_kind": v[-1][3], "n_packed_pairs": v[-1][4], "n_retried_pairs": v[-1][5], "arena_bytes": v[-1][6],
                        "n_main_launches": v[-1][7]}
        out["records_equal"] = True
        print(json.dumps(out), flush=True)
        for lb in libs.values():
            lb.close()


if __name__ == "__main__":
    main()
