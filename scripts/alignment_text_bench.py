"""The display rows on the device (KERNELS.md 4q) measured, in one process on one GPU.  One JSON line per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1, global), generated and
aligned on the device (wfahip_generate_pairs_device, wfahip_align_batch_device).  Every figure is the median of --steps runs after one
warm-up; the shader clock under load (wfahip_debug_clock) is recorded beside them.

  device   wfahip_alignment_text_device on the resident records, ops and sequences, full and trimmed: wall ms of the call, hipEvent ms
           of wfa_altext_len_kernel, of the scan's kernels and of wfa_altext_write_kernel (the library prints them under
           WFAHIP_DEBUG_TIMING=1; this script reads them back from its own stderr); the same with the three planes one byte off a
           4-byte boundary, which is the write kernel's byte-store path (the A/B of its stores); and a device-to-device copy of as many
           bytes as the three planes hold -- the yardstick of the write kernel
  host     wfahip_alignment_text over the same data in host memory, 16 threads and 1 thread, and whether its bytes equal the device's

    python scripts/alignment_text_bench.py [--pairs 1000000] [--steps 5] [--parts device,host]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cigar_text_bench import StderrCapture, clock, med  # noqa: E402


def set_aside(al, L, rec, ops, seqs, q_off, q_len, t_off, t_len, q_rc=None):
    """(records, indices): a copy of rec in which the OK pairs the untrimmed rows cannot be rendered for are marked not OK, and their
    indices.  Under wf-adaptive the reference itself returns ops that consume a base more than a sequence holds now and then
    (KERNELS.md 4q: one pair of this batch), the text entries refuse a batch that holds one -- the reference would index out of
    range -- and a caller that wants the other pairs' rows sets the pair aside like this, on the device: the check under the mask
    NO_ROWS names the pairs (wfahip_check_alignments_device; seqs the blob, or with q_rc the packed words), its pass array goes over
    the records' status column."""
    if q_rc is None:
        _chk, passed, n_flagged = al.check_tensors(rec, ops, seqs, q_off, q_len, t_off, t_len, mask=L.CHK_NO_ROWS)
    else:
        _chk, passed, n_flagged = al.check_tensors_packed(rec, ops, seqs, q_off, q_len, t_off, t_len, q_rc=q_rc, mask=L.CHK_NO_ROWS)
    idx = (passed == L.PAIR_CHECK_FAILED).nonzero().flatten()
    assert idx.numel() == n_flagged
    rec = rec.clone()
    rec[:, L.REC_STATUS] = passed  # (any status but OK: the pair's rows are empty)
    return rec, [int(i) for i in idx.cpu()]


def timed_calls(args, torch, al, ins, only, out):
    """wall ms and the three hipEvent times of --steps calls that write into `out`"""
    wall, ev = [], {"len": [], "scan": [], "write": []}
    for _ in range(args.steps):
        torch.cuda.synchronize()
        with StderrCapture() as cap:
            t0 = time.perf_counter()
            al.alignment_text_tensors(*ins, only_aligned=only, out=out)
            wall.append((time.perf_counter() - t0) * 1e3)
        m = re.search(r"alignment text: .*len ([\d.]+) ms, scan ([\d.]+) ms, write ([\d.]+) ms", cap.text)
        assert m, cap.text
        for k, v in zip(("len", "scan", "write"), m.groups()):
            ev[k].append(float(v))
    return wall, ev


def device_part(args, L, torch, al, ins):
    rec = ins[0]
    n = rec.shape[0]
    os.environ["WFAHIP_DEBUG_TIMING"] = "1"  # (this part only: the diagnostics cost the host entries a synchronisation)
    out = {"part": "device", "pairs": n, "steps": args.steps, **clock(al, L)}
    n_ops = int(rec[:, L.REC_OPS_LEN][rec[:, L.REC_STATUS] == 0].sum(dtype=torch.int64))
    out["ops_per_pair"] = round(n_ops / n, 2)
    for only in (False, True):
        q_row, a_row, t_row, off = al.alignment_text_tensors(*ins, only_aligned=only)  # the warm-up, and the buffers of the timed calls
        total = int(off[-1])
        wall, ev = timed_calls(args, torch, al, ins, only, (q_row, a_row, t_row, off))
        del q_row, a_row, t_row
        odd = [torch.empty(total + 4, dtype=torch.uint8, device=rec.device)[1:1 + total] for _ in range(3)]
        al.alignment_text_tensors(*ins, only_aligned=only, out=(*odd, off))
        _wall, ev_bytes = timed_calls(args, torch, al, ins, only, (*odd, off))
        del odd
        src, dst = (torch.empty(3 * total, dtype=torch.uint8, device=rec.device) for _ in range(2))
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
        del src, dst
        out["trimmed" if only else "full"] = {
            "row_bytes": total, "row_bytes_per_pair": round(total / n, 2), "bytes_written": 3 * total, "call_wall_ms": med(wall),
            "len_kernel_ms": med(ev["len"]), "scan_kernels_ms": med(ev["scan"]), "write_kernel_ms": med(ev["write"]),
            "three_passes_ms": round(med(ev["len"]) + med(ev["scan"]) + med(ev["write"]), 4),
            "len_kernel_ms_all": ev["len"], "write_kernel_ms_all": ev["write"],
            "write_kernel_byte_stores_ms": med(ev_bytes["write"]), "write_kernel_byte_stores_ms_all": ev_bytes["write"],
            "d2d_copy_same_bytes_ms": med(d2d), "d2d_copy_ms_all": [round(x, 4) for x in d2d],
            "write_kernel_over_copy": round(med(ev["write"]) / med(d2d), 2)}
    del os.environ["WFAHIP_DEBUG_TIMING"]
    print(json.dumps(out), flush=True)


def host_part(args, w, L, torch, al, ins):
    rec, ops, blob, q_off, q_len, t_off, t_len = ins
    r = rec.cpu().numpy().view(np.uint32)
    status = r[:, L.REC_STATUS].astype(np.int32)
    ops_len = np.ascontiguousarray(r[:, L.REC_OPS_LEN])
    ops_off = r[:, L.REC_OPS_OFF_LO].astype(np.uint64) | (r[:, L.REC_OPS_OFF_HI].astype(np.uint64) << np.uint64(32))
    z = np.zeros(len(status), np.uint32)
    win = [np.ascontiguousarray(r[:, k]).view(np.int32) for k in (L.REC_TBEGIN, L.REC_TEND, L.REC_QBEGIN, L.REC_QEND)]
    end = int((ops_off + ops_len)[status == 0].max()) if (status == 0).any() else 0  # (the op buffer has slack behind the last pair's ops)
    br = w.BatchResult(status, z, *win, z, z, z, z, ops_off, ops_len, ops[:end].cpu().numpy().view(np.uint64))
    seqs = (blob.cpu().numpy(), q_off.cpu().numpy().view(np.uint64), q_len.cpu().numpy().view(np.uint32),
            t_off.cpu().numpy().view(np.uint64), t_len.cpu().numpy().view(np.uint32))
    out = {"part": "host", "pairs": len(status), "steps": args.steps}
    for only in (False, True):
        key = "trimmed" if only else "full"
        for thr in (16, 1):
            w.alignment_text(br, *seqs, only_aligned=only, n_threads=thr)
            ms = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                host = w.alignment_text(br, *seqs, only_aligned=only, n_threads=thr)
                ms.append((time.perf_counter() - t0) * 1e3)
            out[f"{key}_{thr}_threads_ms"] = med(ms)
            out[f"{key}_{thr}_threads_ms_all"] = [round(x, 1) for x in ms]
        dev = al.alignment_text_tensors(*ins, only_aligned=only)
        out[f"{key}_row_bytes"] = int(host[3][-1])
        out[f"{key}_device_rows_equal_host_rows"] = bool(all(np.array_equal(h.view(np.uint8), d.cpu().numpy().view(np.uint8))
                                                             for h, d in zip(host, dev)))
        del host, dev
    out["note"] = "wall ms through the Python wrapper, which copies the three rows into numpy arrays"
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parts", default="device,host")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("alignment_text_bench: no GPU")
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first: see generate_pairs_device)
    import wfa_amd as w
    from wfa_amd import _lib as L
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
    assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
    d = w.generate_pairs_device(al, 3, args.pairs, 1000, 0.05)
    with StderrCapture():
        rec, ops = al.align_tensors(*d)
    rec, aside = set_aside(al, L, rec, ops, *d)
    print(json.dumps({"part": "input", "pairs": args.pairs, "pairs_set_aside_because_their_ops_overrun_a_sequence": aside}), flush=True)
    ins = (rec, ops, *d)
    if "device" in parts:
        device_part(args, L, torch, al, ins)
    if "host" in parts:
        host_part(args, w, L, torch, al, ins)
    w.RecycleAligner(al)


if __name__ == "__main__":
    main()
