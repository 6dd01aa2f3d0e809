"""The pileup on the device (KERNELS.md 4w) measured at depth 1 and at depth 64, next to the display rows, in one process on one GPU.
One JSON line per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1, global), generated and
aligned on the device; the one pair whose ops overrun its sequences is set aside through check_tensors, as
scripts/alignment_text_bench.py does.  The pileup never reads a target base, so the targets are RE-POINTED by repeating t_off: pair i
faces the region of `pitch` bases at (i // depth) * pitch of the blob (of the words), its own t_len kept -- depth 1 gives every pair
a region of its own (1e6 x 1 088 bases, 35 GB of counters), depth 64 lets 64 alignments meet on every base (544 MB).  The window is
exactly those regions.  Every device figure is the median of --steps timed calls after a warm-up, all of them listed; the times are
the library's own hipEvent times of the two passes (WFAHIP_DEBUG_TIMING=1, read back from this process's stderr).  The counters are
not cleared between calls: the entries add.

  bytes    records of align_tensors: wfahip_pileup_device at both depths, full and trimmed, and wfahip_alignment_text_device on the
           same records in the same loop
  words    records of align_tensors_packed, every second query flagged: wfahip_pileup_packed_device the same way
  host     wfahip_pileup over the same data in host memory at depth 64, 16 threads and 1 thread, and whether its counters equal the
           device's

    python scripts/pileup_bench.py [--pairs 1000000] [--steps 7] [--host-steps 3] [--parts bytes,words,host] [--depths 1,64]
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
from alignment_text_bench import set_aside  # noqa: E402
from alignment_text_packed_bench import PASSES, one_call, store_flagged_reversed  # noqa: E402
from cigar_text_bench import StderrCapture, clock, med  # noqa: E402


def pile_call(torch, call, tag):
    """(n_piled, {pass: hipEvent ms}) of one pileup"""
    torch.cuda.synchronize()
    with StderrCapture() as cap:
        _counts, piled = call()
    m = re.search(tag + r": .*len ([\d.]+) ms, pile ([\d.]+) ms", cap.text)
    assert m, cap.text
    return piled, {"len": float(m.group(1)), "pile": float(m.group(2))}


def repointed(torch, t_len, depth, unit):
    """(t_off int64, pitch, regions): pair i faces region i // depth; unit: bases a step of the offset stands for (1 byte, 16 a word)"""
    n = t_len.numel()
    pitch = -(-(int(t_len.max()) + 16) // 64) * 64          # bases; a multiple of 16, with the pad word's room behind a packed target
    regions = -(-n // depth)
    t_off = (torch.arange(n, device=t_len.device, dtype=torch.int64) // depth) * (pitch // unit)
    return t_off, pitch, regions


def depths_part(args, torch, pile, t_len, unit, size, tag):
    """pile(t_off, pile_n, only, out) is the wrapper's call; size the blob's bytes or the words' number"""
    res = {}
    for depth in args.depths:
        t_off, pitch, regions = repointed(torch, t_len, depth, unit)
        pile_n = regions * pitch
        assert pile_n <= size * unit, "the regions lie inside the blob"
        try:
            counts = torch.zeros((pile_n, 8), dtype=torch.int32, device=t_len.device)
        except torch.OutOfMemoryError:
            res[f"depth_{depth}"] = {"window_bases": pile_n, "counter_bytes": 32 * pile_n, "skipped": "no memory for the counters"}
            continue
        for only in (False, True):
            piled, _ = pile_call(torch, lambda: pile(t_off, pile_n, only, counts), tag)   # the warm-up
            ev = {"len": [], "pile": []}
            for _ in range(args.steps):
                _, e = pile_call(torch, lambda: pile(t_off, pile_n, only, counts), tag)
                for p in ev:
                    ev[p].append(e[p])
            two = [round(a + b, 4) for a, b in zip(ev["len"], ev["pile"])]
            res[f"depth_{depth}_{'trimmed' if only else 'full'}"] = {
                "pairs_piled": piled, "window_bases": pile_n, "counter_bytes": 32 * pile_n, "len_ms": med(ev["len"]), "pile_ms": med(ev["pile"]),
                "two_passes_ms": med(two), "two_passes_ms_all": two, "pile_ms_all": ev["pile"]}
        # what the adds amount to: the mean over the calls, full and trimmed, that went into these counters
        calls = 2 * (args.steps + 1)
        res[f"depth_{depth}_column_adds_per_call"] = int(counts[:, :6].sum(dtype=torch.int64)) // calls
        del counts
        torch.cuda.empty_cache()
    return res


def rows_part(args, torch, rows, tag):
    out = rows(False, None)
    three = []
    for _ in range(args.steps):
        _wall, e = one_call(torch, lambda: rows(False, out), tag)
        three.append(round(sum(e[p] for p in PASSES), 4))
    return {"rows_three_passes_ms": med(three), "rows_three_passes_ms_all": three, "rows_bytes_per_pair": round(3 * int(out[3][-1]) / (out[3].numel() - 1), 1)}


def host_part(args, torch, w, L, al, ins):
    rec, ops, blob, q_off, q_len, _t_off, t_len = ins
    depth = 64
    t_off, pitch, regions = repointed(torch, t_len, depth, 1)
    pile_n = regions * pitch
    r = rec.cpu().numpy().view(np.uint32)
    status = r[:, L.REC_STATUS].astype(np.int32)
    ops_len = np.ascontiguousarray(r[:, L.REC_OPS_LEN])
    ops_off = r[:, L.REC_OPS_OFF_LO].astype(np.uint64) | (r[:, L.REC_OPS_OFF_HI].astype(np.uint64) << np.uint64(32))
    z = np.zeros(len(status), np.uint32)
    win = [np.ascontiguousarray(r[:, k]).view(np.int32) for k in (L.REC_TBEGIN, L.REC_TEND, L.REC_QBEGIN, L.REC_QEND)]
    end = int((ops_off + ops_len)[status == 0].max()) if (status == 0).any() else 0  # (the op buffer has slack behind the last pair's ops)
    br = w.BatchResult(status, z, *win, z, z, z, z, ops_off, ops_len, ops[:end].cpu().numpy().view(np.uint64))
    seqs = (blob.cpu().numpy(), q_off.cpu().numpy().view(np.uint64), q_len.cpu().numpy().view(np.uint32), t_off.cpu().numpy().view(np.uint64),
            t_len.cpu().numpy().view(np.uint32))
    out = {"part": "host", "pairs": len(status), "depth": depth, "window_bases": pile_n, "steps": args.host_steps}
    for only in (False, True):
        key = "trimmed" if only else "full"
        for thr in (16, 1):
            host = np.zeros((pile_n, 8), np.uint32)
            ms = []
            for _ in range(args.host_steps if thr == 16 else 1):
                host[:] = 0
                t0 = time.perf_counter()
                w.pileup(br, *seqs, 0, pile_n, only_aligned=only, n_threads=thr, out=host)
                ms.append((time.perf_counter() - t0) * 1e3)
            out[f"{key}_{thr}_threads_ms"] = med(ms)
            out[f"{key}_{thr}_threads_ms_all"] = [round(x, 1) for x in ms]
        dev, _ = al.pileup_tensors(rec, ops, blob, q_off, q_len, t_off, t_len, 0, pile_n, only_aligned=only)
        out[f"{key}_device_counters_equal_host_counters"] = bool(np.array_equal(host, dev.cpu().numpy().view(np.uint32)))
        del host, dev
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--parts", default="bytes,words,host")
    ap.add_argument("--depths", default="1,64")
    args = ap.parse_args()
    args.depths = [int(d) for d in args.depths.split(",")]
    parts = set(args.parts.split(","))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pileup_bench: no GPU")
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
        if "bytes" in parts:
            os.environ["WFAHIP_DEBUG_TIMING"] = "1"
            res = depths_part(args, torch, lambda t_off2, pile_n, only, out: al.pileup_tensors(rec, ops, blob, q_off, q_len, t_off2, t_len, 0,
                                                                                              pile_n, only_aligned=only, out=out),
                              t_len, 1, blob.numel(), "pileup")
            res.update(rows_part(args, torch, lambda only, out: al.alignment_text_tensors(rec, ops, *d, only_aligned=only, out=out),
                                 "alignment text"))
            del os.environ["WFAHIP_DEBUG_TIMING"]
            print(json.dumps({"part": "bytes", "pairs": args.pairs, "steps": args.steps, "pairs_set_aside": aside, **clock(al, L), **res}),
                  flush=True)
        if "host" in parts:
            host_part(args, torch, w, L, al, (rec, ops, *d))
        del rec, ops
    if "words" in parts:
        q_rc = (torch.arange(args.pairs, device=blob.device) & 1).to(torch.uint8)
        stored = store_flagged_reversed(torch, blob, q_off, q_len, q_rc)
        packed, q_woff, t_woff = al.pack_tensors(stored, q_off, q_len, t_off, t_len)
        del stored
        with StderrCapture():
            rec, ops = al.align_tensors_packed(packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
        rec, aside = set_aside(al, L, rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
        os.environ["WFAHIP_DEBUG_TIMING"] = "1"
        res = depths_part(args, torch, lambda t_woff2, pile_n, only, out: al.pileup_tensors_packed(rec, ops, packed, q_woff, q_len, t_woff2, t_len,
                                                                                                   0, pile_n, q_rc=q_rc, only_aligned=only,
                                                                                                   out=out),
                          t_len, 16, packed.numel(), "pileup packed")
        del os.environ["WFAHIP_DEBUG_TIMING"]
        print(json.dumps({"part": "words", "pairs": args.pairs, "steps": args.steps, "flagged": int(q_rc.sum()), "pairs_set_aside": aside,
                          **clock(al, L), **res}), flush=True)
    w.RecycleAligner(al)


if __name__ == "__main__":
    main()
