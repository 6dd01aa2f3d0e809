"""CIGAR text on the device (KERNELS.md 4p) measured, in one process on one GPU.  One JSON line per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1, global), generated and
aligned on the device (wfahip_generate_pairs_device, wfahip_align_batch_device).  Every figure is the median of --steps runs after one
warm-up; the shader clock under load (wfahip_debug_clock) is recorded beside them.

  device   wfahip_cigar_text_device on the resident records and ops: wall ms of the call, hipEvent ms of wfa_cigar_len_kernel, of the
           scan's kernels and of wfa_cigar_write_kernel (the library prints them under WFAHIP_DEBUG_TIMING=1; this script reads them
           back from its own stderr), the text bytes per pair against the op bytes per pair, and a device-to-device copy of as many
           bytes as the text has -- the yardstick of the write kernel
  host     wfahip_cigar_text over the same ops in host memory, 16 threads and 1 thread (the single-threaded C++ baseline)
  entry    host to host: wfahip_align_batch_text against wfahip_align_batch followed by wfahip_cigar_text (16 threads)

    python scripts/cigar_text_bench.py [--pairs 1000000] [--steps 5] [--parts device,host,entry]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StderrCapture:
    """the library's diagnostics go to the C stderr: file descriptor 2 points at a temporary file while a call runs"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.keep = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.keep, 2)
        os.close(self.keep)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def med(v):
    return round(float(np.median(v)), 4)


def clock(al, L):
    mhz, lo, hi = C.c_double(), C.c_double(), C.c_double()
    L.check(L.lib().wfahip_debug_clock(al._ctx, C.byref(mhz), C.byref(lo), C.byref(hi)), "wfahip_debug_clock")
    return {"shader_mhz": round(mhz.value, 1), "shader_mhz_min": round(lo.value, 1), "shader_mhz_max": round(hi.value, 1)}


def device_part(args, w, L, torch, al, rec, ops):
    n = rec.shape[0]
    os.environ["WFAHIP_DEBUG_TIMING"] = "1"  # (this part only: the diagnostics cost the host entries a synchronisation)
    out = {"part": "device", "pairs": n, "steps": args.steps, **clock(al, L)}
    st = rec[:, L.REC_STATUS] == 0
    n_ops = int(rec[:, L.REC_OPS_LEN][st].sum(dtype=torch.int64))
    out["ops_per_pair"] = round(n_ops / n, 2)
    out["op_bytes_per_pair"] = round(8 * n_ops / n, 1)
    for only in (False, True):
        text, off = al.cigar_tensors(rec, ops, only_aligned=only)  # the warm-up, and the buffers of the timed calls
        total = int(off[-1])
        wall, ev = [], {"len": [], "scan": [], "write": []}
        for _ in range(args.steps):
            torch.cuda.synchronize()
            with StderrCapture() as cap:
                t0 = time.perf_counter()
                al.cigar_tensors(rec, ops, only_aligned=only, out=(text, off))
                wall.append((time.perf_counter() - t0) * 1e3)
            m = re.search(r"cigar text: .*len ([\d.]+) ms, scan ([\d.]+) ms, write ([\d.]+) ms", cap.text)
            assert m, cap.text
            for k, v in zip(("len", "scan", "write"), m.groups()):
                ev[k].append(float(v))
        src, dst = torch.empty(total, dtype=torch.uint8, device=rec.device), torch.empty(total, dtype=torch.uint8, device=rec.device)
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
        key = "trimmed" if only else "full"
        out[key] = {"text_bytes": total, "text_bytes_per_pair": round(total / n, 2), "call_wall_ms": med(wall),
                    "len_kernel_ms": med(ev["len"]), "scan_kernels_ms": med(ev["scan"]), "write_kernel_ms": med(ev["write"]),
                    "three_passes_ms": round(med(ev["len"]) + med(ev["scan"]) + med(ev["write"]), 4),
                    "write_kernel_ms_all": ev["write"], "d2d_copy_same_bytes_ms": med(d2d), "d2d_copy_ms_all": [round(x, 4) for x in d2d]}
        del src, dst
    del os.environ["WFAHIP_DEBUG_TIMING"]
    print(json.dumps(out), flush=True)


def host_part(args, w, L, torch, rec, ops):
    r = rec.cpu().numpy().view(np.uint32)
    status = r[:, L.REC_STATUS].astype(np.int32)
    ops_len = np.ascontiguousarray(r[:, L.REC_OPS_LEN])
    ops_off = r[:, L.REC_OPS_OFF_LO].astype(np.uint64) | (r[:, L.REC_OPS_OFF_HI].astype(np.uint64) << np.uint64(32))
    z = np.zeros(len(status), np.uint32)
    end = int((ops_off + ops_len)[status == 0].max()) if (status == 0).any() else 0  # (the op buffer has slack behind the last pair's ops)
    br = w.BatchResult(status, z, z, z, z, z, z, z, z, z, ops_off, ops_len, ops[:end].cpu().numpy().view(np.uint64))
    out = {"part": "host", "pairs": len(status), "steps": args.steps}
    for thr in (16, 1):
        w.cigar_text(br, n_threads=thr)
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            text, off = w.cigar_text(br, n_threads=thr)
            ms.append((time.perf_counter() - t0) * 1e3)
        out[f"cigar_text_{thr}_threads_ms"] = med(ms)
        out[f"cigar_text_{thr}_threads_ms_all"] = [round(x, 1) for x in ms]
    out["text_bytes"] = int(off[-1])
    print(json.dumps(out), flush=True)
    return text, off


def entry_part(args, w, L, al):
    arrays = w.generate_pairs(3, args.pairs, 1000, 0.05, n_threads=16)

    def two_steps():
        br = al.align_arrays(*arrays)
        return w.cigar_text(br, n_threads=16)

    def one_entry():
        _, text, off = al.align_arrays_text(*arrays)
        return text, off
    legs = {"align_batch_then_cigar_text_16": two_steps, "align_batch_text": one_entry}
    res = {k: f() for k, f in legs.items()}  # the warm-up
    a, b = res.values()
    equal = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    ms = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, f in legs.items():
            with StderrCapture():
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"part": "entry", "pairs": args.pairs, "steps": args.steps, "text_equal": equal,
           "note": "wall ms host to host, through the Python wrappers (both legs copy their results into numpy arrays)"}
    for k, v in ms.items():
        out[k + "_ms"] = med(v)
        out[k + "_ms_all"] = [round(x, 1) for x in v]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parts", default="device,host,entry")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cigar_text_bench: no GPU")
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first: see generate_pairs_device)
    import wfa_amd as w
    from wfa_amd import _lib as L
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
    assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
    if parts & {"device", "host"}:
        d = w.generate_pairs_device(al, 3, args.pairs, 1000, 0.05)
        with StderrCapture():
            rec, ops = al.align_tensors(*d)
        del d
        if "device" in parts:
            device_part(args, w, L, torch, al, rec, ops)
        if "host" in parts:
            text, off = host_part(args, w, L, torch, rec, ops)
            dt, do = al.cigar_tensors(rec, ops)
            same = bool(np.array_equal(dt.cpu().numpy(), text) and np.array_equal(do.cpu().numpy().view(np.uint64), off))
            print(json.dumps({"part": "check", "device_text_equals_host_text": same}), flush=True)
        del rec, ops
        torch.cuda.empty_cache()
    if "entry" in parts:
        entry_part(args, w, L, al)
    w.RecycleAligner(al)


if __name__ == "__main__":
    main()
