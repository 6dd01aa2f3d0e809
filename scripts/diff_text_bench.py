"""The difference string on the device (KERNELS.md 4v) measured against the display rows, in one process on one GPU.  One JSON line
per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1, global), generated and
aligned on the device.  The one pair whose ops overrun its sequences is set aside through check_tensors, as
scripts/alignment_text_bench.py does.  Every device figure is the median of --steps timed calls after a warm-up, all of them listed;
the times are the library's own hipEvent times of the three passes (WFAHIP_DEBUG_TIMING=1, read back from this process's stderr).

  bytes    records of align_tensors: wfahip_diff_text_device and, in the same loop on the same input, wfahip_alignment_text_device --
           full and trimmed; the bytes a pair of the difference string, of the CIGAR text and of the rows
  words    records of align_tensors_packed, every second query flagged: wfahip_diff_text_packed_device against
           wfahip_alignment_text_packed_device, the same way
  host     wfahip_diff_text over the same data in host memory, 16 threads and 1 thread, and whether its bytes equal the device's

    python scripts/diff_text_bench.py [--pairs 1000000] [--steps 7] [--host-steps 3] [--parts bytes,words,host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from alignment_text_bench import set_aside  # noqa: E402
from alignment_text_packed_bench import PASSES, one_call, store_flagged_reversed  # noqa: E402
from cigar_text_bench import StderrCapture, clock, med  # noqa: E402


def compare(args, torch, L, al, rec, ops, diff, rows, diff_tag, rows_tag):
    """diff(only, out) / rows(only, out) render into out (None: sized by the call); the tags are what the library prints before its
    times.  Returns the figures of both modes."""
    n = rec.shape[0]
    res = {}
    for only in (False, True):
        d_out = diff(only, None)     # the warm-up, and the buffers of the timed calls
        r_out = rows(only, None)
        ev = {"diff": {p: [] for p in PASSES}, "rows": {p: [] for p in PASSES}}
        for _ in range(args.steps):  # interleaved: both see the same clocks
            for key, f, out, tag in (("diff", diff, d_out, diff_tag), ("rows", rows, r_out, rows_tag)):
                _wall, e = one_call(torch, lambda: f(only, out), tag)
                for p in PASSES:
                    ev[key][p].append(e[p])
        three = {k: [round(sum(ev[k][p][s] for p in PASSES), 4) for s in range(args.steps)] for k in ev}
        cig_text, cig_off = al.cigar_tensors(rec, ops, only_aligned=only)
        res["trimmed" if only else "full"] = {
            "diff_bytes_per_pair": round(int(d_out[1][-1]) / n, 2), "cigar_text_bytes_per_pair": round(int(cig_off[-1]) / n, 2),
            "rows_bytes_per_pair": round(3 * int(r_out[3][-1]) / n, 2),
            "diff_three_passes_ms": med(three["diff"]), "rows_three_passes_ms": med(three["rows"]),
            "diff_not_slower_than_rows": bool(med(three["diff"]) <= med(three["rows"])),
            "diff_three_passes_ms_all": three["diff"], "rows_three_passes_ms_all": three["rows"],
            **{f"diff_{p}_ms": med(ev["diff"][p]) for p in PASSES}, **{f"rows_{p}_ms": med(ev["rows"][p]) for p in PASSES},
            "diff_write_ms_all": ev["diff"]["write"], "rows_write_ms_all": ev["rows"]["write"]}
        del d_out, r_out, cig_text, cig_off
    return res


def host_part(args, w, L, al, ins):
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
    out = {"part": "host", "pairs": len(status), "steps": args.host_steps}
    for only in (False, True):
        key = "trimmed" if only else "full"
        for thr in (16, 1):
            w.diff_text(br, *seqs, only_aligned=only, n_threads=thr)
            ms = []
            for _ in range(args.host_steps):
                t0 = time.perf_counter()
                host = w.diff_text(br, *seqs, only_aligned=only, n_threads=thr)
                ms.append((time.perf_counter() - t0) * 1e3)
            out[f"{key}_{thr}_threads_ms"] = med(ms)
            out[f"{key}_{thr}_threads_ms_all"] = [round(x, 1) for x in ms]
        dev = al.diff_tensors(*ins, only_aligned=only)
        out[f"{key}_bytes"] = int(host[1][-1])
        out[f"{key}_device_text_equals_host_text"] = bool(all(np.array_equal(h.view(np.uint8), d.cpu().numpy().view(np.uint8))
                                                              for h, d in zip(host, dev)))
        del host, dev
    out["note"] = "wall ms through the Python wrapper, which copies the text into a numpy array"
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--parts", default="bytes,words,host")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("diff_text_bench: no GPU")
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first: see generate_pairs_device)
    import wfa_amd as w
    from wfa_amd import _lib as L
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
    assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
    blob, q_off, q_len, t_off, t_len = d = w.generate_pairs_device(al, 3, args.pairs, 1000, 0.05)
    if parts & {"bytes", "host"}:
        with StderrCapture():
            rec, ops = al.align_tensors(*d)
        rec, aside = set_aside(al, L, rec, ops, *d)
        ins = (rec, ops, *d)
        if "bytes" in parts:
            os.environ["WFAHIP_DEBUG_TIMING"] = "1"
            res = compare(args, torch, L, al, rec, ops,
                          lambda only, out: al.diff_tensors(*ins, only_aligned=only, out=out),
                          lambda only, out: al.alignment_text_tensors(*ins, only_aligned=only, out=out), "diff text", "alignment text")
            del os.environ["WFAHIP_DEBUG_TIMING"]
            print(json.dumps({"part": "bytes", "pairs": args.pairs, "steps": args.steps, "pairs_set_aside": aside, **clock(al, L), **res}),
                  flush=True)
        if "host" in parts:
            host_part(args, w, L, al, ins)
        del rec, ops, ins
    if "words" in parts:
        q_rc = (torch.arange(args.pairs, device=blob.device) & 1).to(torch.uint8)
        stored = store_flagged_reversed(torch, blob, q_off, q_len, q_rc)
        packed, q_woff, t_woff = al.pack_tensors(stored, q_off, q_len, t_off, t_len)
        del stored
        with StderrCapture():
            rec, ops = al.align_tensors_packed(packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
        rec, aside = set_aside(al, L, rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
        pk = (rec, ops, packed, q_woff, q_len, t_woff, t_len)
        os.environ["WFAHIP_DEBUG_TIMING"] = "1"
        res = compare(args, torch, L, al, rec, ops,
                      lambda only, out: al.diff_tensors_packed(*pk, q_rc=q_rc, only_aligned=only, out=out),
                      lambda only, out: al.alignment_text_tensors_packed(*pk, q_rc=q_rc, only_aligned=only, out=out),
                      "diff text packed", "alignment text packed")
        del os.environ["WFAHIP_DEBUG_TIMING"]
        print(json.dumps({"part": "words", "pairs": args.pairs, "steps": args.steps, "flagged": int(q_rc.sum()), "pairs_set_aside": aside,
                          **clock(al, L), **res}), flush=True)
    w.RecycleAligner(al)


if __name__ == "__main__":
    main()
