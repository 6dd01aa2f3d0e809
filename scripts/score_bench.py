"""Score-only against full alignment on the same host inputs, in one process (include/wfa_hip.h: wfahip_score_batch vs
wfahip_align_batch).  Workloads as bench.py generates them: c3 = 1e6 x 1 kbp @5 %, seed 3, global, wf-adaptive 10/50/1,
penalties 4/6/2; g3 = the same pairs semi-global.  After a warm-up of each entry, the two calls alternate --steps times;
per entry: pairs/s, wall ms per call (host clock around the synchronous call) and the kernel ms last_timing reports.
The scores of the two entries must agree.  One JSON line per workload.

Long-read legs (wfa_score_long_kernel, KERNELS.md 4i): L5 = 2e4 x 50 kbp @5 %, l5 = 500 x 50 kbp @5 %, global, 4/6/2,
wf-adaptive 10/50/1, seed 5; --pairs scales L5 down for a rehearsal.  --other-lib PATH adds a third leg: wfahip_score_batch of
ANOTHER build of the library (the parent commit's, built beforehand) on the same inputs, alternating with the two others in
the same process, so that the new score path is read against the old one and against that one's own run-to-run spread.

Device leg (--device, KERNELS.md 4j): the legs become `score` (wfahip_score_batch, host arrays), `score_device`
(wfahip_score_batch_device on the same data resident in HBM, results left there) and `align_device`
(wfahip_align_batch_device on the same buffers), alternating per step; the scores of all three are compared in every step,
outside the timed region.

Packed leg (--packed, KERNELS.md 4l): the legs become `score` (wfahip_score_batch on the bytes) and `score_packed`
(wfahip_score_batch_packed on the same pairs, packed ONCE by wfahip_pack_pairs before the steps and timed apart: "pack_ms"),
alternating per step; --other-lib adds the parent's wfahip_score_batch as the yardstick.  Per leg also "upload_bytes_computed": what a
call uploads by the entries' rules (with the default gate of 64 long pairs) -- computed here, not read from the library or a trace.

    python scripts/score_bench.py [--configs c3,g3] [--pairs 1000000] [--steps 5]
    python scripts/score_bench.py --packed --configs c3,g3,L5 [--other-lib parent/wfa_amd/lib/libwfahip.so]
    python scripts/score_bench.py --device --configs c3,g3,L5 [--other-lib parent/wfa_amd/lib/libwfahip.so]
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


def device_legs(w, al, arrays, glob, length, err):
    """The legs on device-resident input: the batch as torch tensors in HBM, scored by wfahip_score_batch_device and aligned by
    wfahip_align_batch_device.  Each returns a function that fetches (status, score) -- called outside the timed region."""
    import torch
    from wfa_amd import _lib as L
    dev = torch.device("cuda", 0)
    blob, q_off, q_len, t_off, t_len = arrays
    n = len(q_len)
    d = [torch.from_numpy(a).to(dev) for a in (blob, q_off.view(np.int64), q_len.view(np.int32), t_off.view(np.int64), t_len.view(np.int32))]
    max_len = int(max(q_len.max(), t_len.max()))
    sum_len = int(q_len.astype(np.int64).sum() + t_len.astype(np.int64).sum())
    ops_cap = int(sum_len * max(0.25, 3.0 * err)) + 8 * n + 1024  # (bench.py's sizing)
    if not glob or length >= 20000:
        ops_cap = sum_len + 2 * n + 1024
    d_rec = torch.zeros((n, L.REC_WORDS), dtype=torch.int32, device=dev)
    d_ops = torch.zeros(ops_cap, dtype=torch.int64, device=dev)
    out = (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    prm, lib = al._params(), L.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def score_device():
        al.score_tensors(*d, out=out)
        return lambda: (out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32))

    def align_device():
        needed = C.c_uint64()
        L.check(lib.wfahip_align_batch_device(al._ctx, C.byref(prm), d[0].data_ptr(), blob.size, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                              d[4].data_ptr(), n, max_len, d_rec.data_ptr(), d_ops.data_ptr(), ops_cap, C.byref(needed), stream),
                "wfahip_align_batch_device")

        def fetch():
            rec = d_rec[:, :2].cpu().numpy()
            st = rec[:, L.REC_STATUS].copy()
            return st, np.where(st == 0, rec[:, L.REC_SCORE].view(np.uint32), 0).astype(np.uint32)
        return fetch

    return [("score_device", score_device, al), ("align_device", align_device, al)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,g3")
    ap.add_argument("--pairs", type=int, default=None, help="pairs of c3 / g3 (default 1e6); scales L5 down when given")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--device", action="store_true", help="legs on device-resident input: score (host entry), score_device, align_device")
    ap.add_argument("--packed", action="store_true", help="legs on 2-bit packed input: score (bytes) and score_packed, packed once")
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
        if args.device:
            fns = [("score", lambda: al.score_arrays(*arrays), al)] + device_legs(w, al, arrays, glob, length, err)
        extra, upload = {}, {}
        if args.packed:
            t0 = time.perf_counter()
            packed, q_woff, t_woff = w.pack_pairs(*arrays, n_threads=16)
            extra["pack_ms"] = (time.perf_counter() - t0) * 1e3
            pk = (packed, q_woff, arrays[2], t_woff, arrays[4])
            fns = [("score", lambda: al.score_arrays(*arrays), al), ("score_packed", lambda: al.score_arrays_packed(*pk), al)]
            # bytes a call uploads: the blob or the words, the two offset and the two length arrays (none when every pair is long),
            # and for the global pairs beyond 2 047 bases their table -- and, in the byte entry, their words, which it packs itself
            lng = (np.maximum(arrays[2], arrays[4]) > 2047) if glob else np.zeros(pairs, bool)
            n_long = int(lng.sum()) if lng.sum() >= 64 else 0
            long_words = int((((arrays[2][lng].astype(np.int64) + 15) // 16 + 1) + ((arrays[4][lng].astype(np.int64) + 15) // 16 + 1)).sum()) if n_long else 0
            n_arr = 0 if n_long == pairs else 24 * pairs
            by = (0 if n_long == pairs else int(arrays[0].size)) + n_arr + 4 * long_words + 32 * n_long
            upload = {"score": by, "score_packed": 4 * int(packed.size) + n_arr + 32 * n_long, "score_other": by}
        ref_leg = "score" if args.device or args.packed else "align"
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
            if args.device or args.packed:
                ref_status, want = res["score"]
            else:
                ref_status, want = res["align"].status, np.where(res["align"].status == 0, res["align"].score, 0)
            for leg in legs:  # the scores are compared in every step
                if leg != ref_leg:
                    st, sc = res[leg]() if callable(res[leg]) else res[leg]
                    assert np.array_equal(st, ref_status) and np.array_equal(sc, want), (name, leg)
        out = {"config": name, "pairs": pairs, "steps": args.steps, **extra}
        for leg, v in legs.items():
            wall = float(np.median([x[0] for x in v]))
            out[leg] = {"pairs_per_s": pairs / wall * 1e3, "wall_ms": wall, "kernel_ms": float(np.median([x[1] for x in v])),
                        "main_kernel_kind": v[-1][2], "n_retried_pairs": v[-1][3], "arena_bytes": v[-1][4],
                        "wall_ms_all": [round(x[0], 2) for x in v], "wall_ms_spread": round(max(x[0] for x in v) - min(x[0] for x in v), 2)}
            if leg in upload:
                out[leg]["upload_bytes_computed"] = upload[leg]
            out[leg]["kernel_ms_all"] = [round(x[1], 2) for x in v]
        out["scores_equal"] = True
        print(json.dumps(out), flush=True)
        if other:
            other.close()
        w.RecycleAligner(al)


if __name__ == "__main__":
    main()
