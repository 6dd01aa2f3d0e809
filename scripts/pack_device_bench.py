"""The packed entries on device-resident input (KERNELS.md 4r) measured, in one process on one GPU.  One JSON line per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1, global), generated on the
device (wfahip_generate_pairs_device).  Every figure is the median of --steps runs after one warm-up.

  pack     wfahip_pack_pairs_device: wall ms of the call and hipEvent ms of its three passes (the library prints them under
           WFAHIP_DEBUG_TIMING=1; this script reads them back from its own stderr); a device-to-device copy of the blob's bytes as
           the floor -- the pack pass reads those bytes once and writes a quarter of them --; and wfahip_pack_pairs over the same bytes
           in host memory on 16 threads.  The words of the two packers are compared.  The generator lays every sequence at a multiple of
           16 bytes, so the pack pass takes its 16-byte loads throughout; it is timed once more on a copy of the blob five bytes off such a
           boundary, where every piece is read in aligned dwords.
  align    wfahip_align_batch_packed_device on the resident words, against wfahip_align_batch_packed host to host on the same words
           and against wfahip_align_batch_device on the resident bytes: wall ms of each call

    python scripts/pack_device_bench.py [--pairs 1000000] [--steps 5] [--parts pack,align]
"""
import argparse
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


def pack_part(args, w, torch, al, d):
    blob = d[0]
    os.environ["WFAHIP_DEBUG_TIMING"] = "1"  # (this part only)
    with StderrCapture():
        packed, q_woff, t_woff = al.pack_tensors(*d)  # the warm-up
    wall, ev = [], {"len": [], "scan": [], "pack": []}
    for _ in range(args.steps):
        torch.cuda.synchronize()
        with StderrCapture() as cap:
            t0 = time.perf_counter()
            al.pack_tensors(*d)
            wall.append((time.perf_counter() - t0) * 1e3)
        m = re.search(r"pack pairs: .*len ([\d.]+) ms, scan ([\d.]+) ms, pack ([\d.]+) ms", cap.text)
        assert m, cap.text
        for k, v in zip(("len", "scan", "pack"), m.groups()):
            ev[k].append(float(v))
    # the same bytes five bytes off a 16-byte boundary: every piece takes the aligned-dword path in place of the 16-byte load
    room = torch.empty(blob.numel() + 16, dtype=torch.uint8, device=blob.device)
    off5 = room[5:5 + blob.numel()]
    off5.copy_(blob)
    ev5 = []
    for k in range(args.steps + 1):
        torch.cuda.synchronize()
        with StderrCapture() as cap:
            p5 = al.pack_tensors(off5, *d[1:])[0]
        m = re.search(r"pack pairs: .*pack ([\d.]+) ms", cap.text)
        assert m, cap.text
        if k:
            ev5.append(float(m.group(1)))
    same5 = bool(torch.equal(p5, packed))
    del room, off5, p5
    del os.environ["WFAHIP_DEBUG_TIMING"]
    dst = torch.empty_like(blob)
    dst.copy_(blob)
    d2d = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        dst.copy_(blob)
        b.record()
        torch.cuda.synchronize()
        d2d.append(a.elapsed_time(b))
    del dst
    host = [t.cpu().numpy() for t in d]
    host = (host[0], host[1].view(np.uint64), host[2].view(np.uint32), host[3].view(np.uint64), host[4].view(np.uint32))
    hp = w.pack_pairs(*host, n_threads=16)
    hms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        w.pack_pairs(*host, n_threads=16)
        hms.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(packed.cpu().numpy().view(np.uint32)[:-4], hp[0]) and np.array_equal(q_woff.cpu().numpy().view(np.uint64), hp[1])
                and np.array_equal(t_woff.cpu().numpy().view(np.uint64), hp[2]))
    three = round(med(ev["len"]) + med(ev["scan"]) + med(ev["pack"]), 4)
    out = {"part": "pack", "pairs": int(d[2].numel()), "steps": args.steps, "blob_bytes": int(blob.numel()), "words": int(packed.numel()) - 4,
           "pack_tensors_wall_ms": med(wall), "note": "pack_tensors makes the sizing call and the real one: the first two passes run twice in its wall time",
           "len_kernel_ms": med(ev["len"]), "scan_kernels_ms": med(ev["scan"]), "pack_kernel_ms": med(ev["pack"]), "three_passes_ms": three,
           "pack_kernel_ms_all": ev["pack"], "pack_kernel_sources_5_bytes_off_ms": med(ev5), "pack_kernel_5_off_ms_all": ev5,
           "words_5_bytes_off_equal": same5, "d2d_copy_blob_ms": med(d2d), "d2d_copy_ms_all": [round(x, 4) for x in d2d],
           "three_passes_over_d2d_copy": round(three / max(med(d2d), 1e-9), 2), "host_pack_pairs_16_threads_ms": med(hms),
           "host_pack_ms_all": [round(x, 1) for x in hms], "device_words_equal_host_words": same}
    print(json.dumps(out), flush=True)
    return (packed, q_woff, t_woff), hp, host


def align_part(args, w, torch, al, d, dev_pk, host_pk, host):
    packed, q_woff, t_woff = dev_pk
    legs = {
        "align_batch_packed_device": lambda: al.align_tensors_packed(packed, q_woff, d[2], t_woff, d[4]),
        "align_batch_device_on_bytes": lambda: al.align_tensors(*d),
        "align_batch_packed_host_to_host": lambda: al.align_arrays_packed(host_pk[0], host_pk[1], host[2], host_pk[2], host[4]),
    }
    res = {}
    for k, f in legs.items():  # the warm-up
        res[k] = f()
        torch.cuda.synchronize()
    st_dev = res["align_batch_packed_device"][0][:, 0].cpu().numpy()
    sc_dev = res["align_batch_packed_device"][0][:, 1].cpu().numpy().view(np.uint32)
    br = res["align_batch_packed_host_to_host"]
    equal = bool(np.array_equal(st_dev, br.status) and np.array_equal(sc_dev, br.score))
    del res
    ms = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            del r
    out = {"part": "align", "pairs": int(d[2].numel()), "steps": args.steps, "status_and_score_equal_host_entry": equal,
           "note": "wall ms through the Python wrappers; the device legs allocate and zero their record and op tensors inside the timed call"}
    for k, v in ms.items():
        out[k + "_ms"] = med(v)
        out[k + "_ms_all"] = [round(x, 1) for x in v]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parts", default="pack,align")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pack_device_bench: no GPU")
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first: see generate_pairs_device)
    import wfa_amd as w
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
    assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
    d = w.generate_pairs_device(al, 3, args.pairs, 1000, 0.05)
    dev_pk, host_pk, host = pack_part(args, w, torch, al, d)
    if "align" in parts:
        align_part(args, w, torch, al, d, dev_pk, host_pk, host)
    w.RecycleAligner(al)


if __name__ == "__main__":
    main()
