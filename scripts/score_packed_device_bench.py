"""The screen on device-resident words (KERNELS.md 4s) measured, in one process on one GPU.  One JSON line per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1), global (c3) and
semi-global (g3).  Half the pairs are flagged: their queries lie reverse-complemented in the packed buffer, so that every pair scores
the bases the generator made.  One warm-up of every leg, then the legs alternate --steps times; per leg the median wall ms of the call
(host clock around the synchronous call), its spread (max - min) and the kernel_ms wfahip_last_timing reports.  Status and score of
the three legs are compared in every step, outside the timed region.

  score    score_packed_device  wfahip_score_batch_packed_device on the words, offsets, lengths and flags resident in HBM
           score_packed_rc      wfahip_score_batch_packed_rc on the same words in host memory
           score_device_bytes   wfahip_score_batch_device on the same bases as bytes resident in HBM (no flags: the forward bytes)
  select   wfahip_select_pairs_device on 2e6 statuses, a random third of them OK, with flags: wall ms of the call into preallocated
           outputs, beside a device-to-device copy of the bytes of its five input arrays and the statuses

    python scripts/score_packed_device_bench.py [--pairs 1000000] [--steps 5] [--parts score,select] [--configs c3,g3]
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

COMP = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    COMP[a] = b


def leg_stats(v):
    wall = [x[0] for x in v]
    return {"wall_ms": round(float(np.median(wall)), 2), "wall_ms_spread": round(max(wall) - min(wall), 2), "wall_ms_all": [round(x, 2) for x in wall],
            "kernel_ms": round(float(np.median([x[1] for x in v])), 2), "kernel_ms_all": [round(x[1], 2) for x in v],
            "main_kernel_kind": v[-1][2], "n_retried_pairs": v[-1][3], "arena_bytes": v[-1][4]}


def score_part(args, w, torch, name, glob):
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=glob), device=0)
    assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
    d = w.generate_pairs_device(al, 3, args.pairs, 1000, 0.05)  # the forward bytes, in HBM
    n = int(d[2].numel())
    flags = (np.arange(n) % 2).astype(np.uint8)
    host = [t.cpu().numpy() for t in d]
    stored = host[0].copy()  # ... and what the packed buffer holds: a flagged pair's query reverse-complemented
    for o, k in zip(host[1][flags != 0], host[2][flags != 0]):
        stored[o:o + k] = COMP[host[0][o:o + k][::-1]]
    d_stored = torch.from_numpy(stored).to(d[0].device)
    packed, q_woff, t_woff = al.pack_tensors(d_stored, *d[1:])
    del d_stored
    d_rc = torch.from_numpy(flags).to(d[0].device)
    h_pk = (packed.cpu().numpy().view(np.uint32)[:-4].copy(), q_woff.cpu().numpy().view(np.uint64), host[2].view(np.uint32),
            t_woff.cpu().numpy().view(np.uint64), host[4].view(np.uint32))
    out_pk = (torch.zeros(n, dtype=torch.int32, device=d[0].device), torch.zeros(n, dtype=torch.int32, device=d[0].device))
    out_by = (torch.zeros_like(out_pk[0]), torch.zeros_like(out_pk[1]))
    fetch = lambda o: (o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint32))

    def score_packed_device():
        al.score_tensors_packed(packed, q_woff, d[2], t_woff, d[4], q_rc=d_rc, out=out_pk)
        return lambda: fetch(out_pk)

    def score_packed_rc():
        r = al.score_arrays_packed_rc(*h_pk, flags)
        return lambda: r

    def score_device_bytes():
        al.score_tensors(*d, out=out_by)
        return lambda: fetch(out_by)

    fns = [("score_packed_device", score_packed_device), ("score_packed_rc", score_packed_rc), ("score_device_bytes", score_device_bytes)]
    for _, fn in fns:
        fn()  # warm-up: buffers, code objects
    legs = {leg: [] for leg, _ in fns}
    for _ in range(args.steps):
        res = {}
        for leg, fn in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[leg] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            t = al.last_timing()
            legs[leg].append((dt, t.kernel_ms, t.main_kernel_kind, t.n_retried_pairs, t.arena_bytes))
        st, sc = res["score_packed_rc"]()
        for leg in ("score_packed_device", "score_device_bytes"):  # the scores are compared in every step
            a, b = res[leg]()
            assert np.array_equal(a, st) and np.array_equal(b, sc), (name, leg)
    out = {"part": "score", "config": name, "pairs": n, "steps": args.steps, "flagged": int(flags.sum()), "words": int(packed.numel()) - 4,
           "scores_equal": True}
    for leg, v in legs.items():
        out[leg] = leg_stats(v)
    print(json.dumps(out), flush=True)
    w.RecycleAligner(al)


def select_part(args, w, torch):
    from wfa_amd import _lib as L
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
    dev = torch.device("cuda", 0)
    n = 2 * args.pairs
    rng = np.random.default_rng(3)
    status = np.where(rng.random(n) < 1 / 3, 0, 8).astype(np.int32)
    ins = [torch.from_numpy(a).to(dev) for a in (status, rng.integers(0, 1 << 40, n), rng.integers(1, 2000, n).astype(np.int32),
                                                 rng.integers(0, 1 << 40, n), rng.integers(1, 2000, n).astype(np.int32),
                                                 rng.integers(0, 2, n).astype(np.uint8))]
    outs = [torch.empty(n, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int32, torch.int64, torch.int32, torch.uint8)]
    cnt = C.c_uint64(0)
    lib = L.lib()

    def call():
        L.check(lib.wfahip_select_pairs_device(al._ctx, *[t.data_ptr() for t in ins[:1]], n, *[t.data_ptr() for t in ins[1:]],
                                               *[t.data_ptr() for t in outs], C.byref(cnt), None), "wfahip_select_pairs_device")
    call()
    keep = np.nonzero(status == 0)[0]
    equal = bool(cnt.value == len(keep) and np.array_equal(outs[0][:len(keep)].cpu().numpy().view(np.uint32), keep.astype(np.uint32))
                 and all(torch.equal(o[:len(keep)], i[torch.from_numpy(keep).to(dev)]) for o, i in zip(outs[1:], ins[1:])))
    ms = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    n_bytes = sum(t.numel() * t.element_size() for t in ins)
    src, dst = torch.empty(n_bytes, dtype=torch.uint8, device=dev), torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    dst.copy_(src)
    d2d = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        d2d.append(a.elapsed_time(b))
    print(json.dumps({"part": "select", "statuses": n, "selected": int(cnt.value), "steps": args.steps, "equals_numpy_nonzero": equal,
                      "select_pairs_device_wall_ms": round(float(np.median(ms)), 4), "select_wall_ms_all": [round(x, 4) for x in ms],
                      "input_bytes": n_bytes, "d2d_copy_same_bytes_ms": round(float(np.median(d2d)), 4),
                      "d2d_copy_ms_all": [round(x, 4) for x in d2d]}), flush=True)
    w.RecycleAligner(al)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parts", default="score,select")
    ap.add_argument("--configs", default="c3,g3")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("score_packed_device_bench: no GPU")
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first: see generate_pairs_device)
    import wfa_amd as w
    parts = set(args.parts.split(","))
    if "score" in parts:
        for name in args.configs.split(","):
            score_part(args, w, torch, name, {"c3": True, "g3": False}[name])
    if "select" in parts:
        select_part(args, w, torch)


if __name__ == "__main__":
    main()
