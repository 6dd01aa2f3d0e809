"""Full alignment under a score bound against the plain entry on the same host inputs, in one process (include/wfa_hip.h:
wfahip_align_batch_bounded vs wfahip_align_batch; KERNELS.md 4k).  Global, wf-adaptive 10/50/1, penalties 4/6/2.

    a   1e6 x 1 kbp @5 %, seed 3 (bench.py's c3), bound 1 000: nothing is rejected -- the bounded call costs one filter launch
        over the records more than the plain one and must sit within the plain call's own spread
    b   5e5 related pairs (seed 32) interleaved with 5e5 unrelated ones (query i of seed 32 against target i of seed 77),
        bound 400: half the batch is rejected

After a warm-up of each entry the two calls alternate --steps times.  Per entry: wall ms per call (host clock around the
synchronous call: median, every step, spread of the repeated identical calls), and from wfahip_last_timing kernel ms, arena
bytes, launches, retried pairs.  In every step the bounded result is compared with the plain one filtered by the bound
(status and score), outside the timed region.  --device adds the two device entries on the same data resident in HBM (no
PCIe in the call).  One JSON line per workload.

    python scripts/bounded_bench.py [--workloads a,b] [--pairs 1000000] [--steps 5] [--device]
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


def mixed(w, n_each, length):
    a = w.generate_pairs(32, n_each, length, 0.05, n_threads=16)
    b = w.generate_pairs(77, n_each, length, 0.05, n_threads=16)
    pad = (-len(a[0])) % 16
    blob = np.concatenate([a[0], np.zeros(pad, np.uint8), b[0]])
    shift = np.uint64(len(a[0]) + pad)
    q_off, q_len = np.repeat(a[1], 2), np.repeat(a[2], 2)
    t_off, t_len = np.empty(2 * n_each, np.uint64), np.empty(2 * n_each, np.uint32)
    t_off[0::2], t_len[0::2] = a[3], a[4]
    t_off[1::2], t_len[1::2] = b[3] + shift, b[4]
    return blob, q_off, q_len, t_off, t_len


def device_legs(al, arrays, bound):
    import torch
    from wfa_amd import _lib as L
    dev = torch.device("cuda", 0)
    blob, q_off, q_len, t_off, t_len = arrays
    n = len(q_len)
    d = [torch.from_numpy(a).to(dev) for a in (blob, q_off.view(np.int64), q_len.view(np.int32), t_off.view(np.int64), t_len.view(np.int32))]
    max_len = int(max(q_len.max(), t_len.max()))
    sum_len = int(q_len.astype(np.int64).sum() + t_len.astype(np.int64).sum())
    # (the plain entry backtraces the unrelated pairs too: a score of 2 300 at 4/6/2 reserves 2 * score / min(x, e) + 8 ops)
    ops_cap = (sum_len // 2 if bound >= 1000 else 2 * sum_len) + 16 * n + 1024
    d_rec = torch.zeros((n, L.REC_WORDS), dtype=torch.int32, device=dev)
    d_ops = torch.zeros(ops_cap, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    prm, lib = al._params(), L.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fetch():
        rec = d_rec[:, :2].cpu().numpy()
        st = rec[:, L.REC_STATUS].copy()
        return st, np.where(st == 0, rec[:, L.REC_SCORE].view(np.uint32), 0).astype(np.uint32)

    def plain():
        needed = C.c_uint64()
        L.check(lib.wfahip_align_batch_device(al._ctx, C.byref(prm), d[0].data_ptr(), blob.size, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                              d[4].data_ptr(), n, max_len, d_rec.data_ptr(), d_ops.data_ptr(), ops_cap, C.byref(needed), stream),
                "wfahip_align_batch_device")
        return fetch

    def bounded():
        needed = C.c_uint64()
        L.check(lib.wfahip_align_batch_bounded_device(al._ctx, C.byref(prm), d[0].data_ptr(), blob.size, d[1].data_ptr(), d[2].data_ptr(),
                                                      d[3].data_ptr(), d[4].data_ptr(), n, max_len, bound, d_rec.data_ptr(), d_ops.data_ptr(), ops_cap,
                                                      C.byref(needed), stream), "wfahip_align_batch_bounded_device")
        return fetch

    return [("plain_device", plain), ("bounded_device", bounded)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--device", action="store_true", help="also the device entries on the same data resident in HBM")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bounded_bench: no GPU")
    import wfa_amd as w
    for name in args.workloads.split(","):
        if name == "a":
            arrays, bound = w.generate_pairs(3, args.pairs, 1000, 0.05, n_threads=16), 1000
        else:
            arrays, bound = mixed(w, args.pairs // 2, 1000), 400
        n = len(arrays[2])
        al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
        assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None

        def host(max_score):
            def fn():
                r = al.align_arrays(*arrays, max_score=max_score)
                return r.status, np.where(r.status == 0, r.score, 0).astype(np.uint32)
            return fn

        fns = [("plain", host(0)), ("bounded", host(bound))]
        if args.device:
            fns += device_legs(al, arrays, bound)
        for _, fn in fns:
            fn()  # warm-up: buffers, code objects, what the context learns
        legs = {leg: [] for leg, _ in fns}
        n_over = 0
        for _ in range(args.steps):
            res = {}
            for leg, fn in fns:
                t0 = time.perf_counter()
                r = fn()
                dt = (time.perf_counter() - t0) * 1e3
                t = al.last_timing()
                legs[leg].append((dt, t.kernel_ms, t.total_ms, t.arena_bytes, t.n_launches, t.n_retried_pairs, t.main_kernel_kind))
                res[leg] = r() if callable(r) else r
            for sfx in ("", "_device") if args.device else ("",):  # the bounded result = the plain one, filtered
                (st0, sc0), (st1, sc1) = res["plain" + sfx], res["bounded" + sfx]
                over = (st0 == 0) & (sc0 > bound)
                n_over = int(over.sum())
                assert np.array_equal(st1, np.where(over, 8, st0)) and np.array_equal(sc1, np.where(over, 0, sc0)), (name, sfx)
        out = {"workload": name, "pairs": n, "bound": bound, "pairs_over": n_over, "steps": args.steps}
        for leg, v in legs.items():
            wall = [x[0] for x in v]
            out[leg] = {"wall_ms": round(float(np.median(wall)), 2), "wall_ms_all": [round(x, 2) for x in wall],
                        "wall_ms_spread": round(max(wall) - min(wall), 2), "kernel_ms": round(float(np.median([x[1] for x in v])), 3),
                        "device_total_ms": round(float(np.median([x[2] for x in v])), 3), "arena_bytes": v[-1][3], "n_launches": v[-1][4],
                        "n_retried_pairs": v[-1][5], "main_kernel_kind": v[-1][6]}
        out["results_equal"] = True
        print(json.dumps(out), flush=True)
        w.RecycleAligner(al)


if __name__ == "__main__":
    main()
