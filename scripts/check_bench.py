"""The check on the device (KERNELS.md 4u) measured, in one process on one GPU.  One JSON line per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1, global), generated and
aligned on the device (wfahip_generate_pairs_device, wfahip_align_batch_device).  Every figure is the median of --steps timed calls
after a warm-up, hipEvent times the library prints under WFAHIP_DEBUG_TIMING=1 (this script reads them back from its own stderr).

  bytes    wfahip_check_alignments_device on the resident records, ops and sequences: the kernel's ms, the flagged pairs by flag and
           their indices; and, in the same run on the same input with the NO_ROWS pairs set aside, the three passes of
           wfahip_alignment_text_device -- the bar the check's kernel must not exceed
  words    wfahip_check_alignments_packed_device over the same pairs as 2-bit words, every second query stored reverse-complemented
           and flagged (wfahip_pack_pairs_device, wfahip_align_batch_packed_device): the kernel's ms and the flagged pairs

    python scripts/check_bench.py [--pairs 1000000] [--steps 5]
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cigar_text_bench import StderrCapture, clock, med  # noqa: E402
from alignment_text_packed_bench import store_flagged_reversed  # noqa: E402


def timed(steps, call, pattern):
    """the groups of `pattern` in the diagnostics of `steps` calls, as lists of floats"""
    out = None
    for _ in range(steps):
        with StderrCapture() as cap:
            call()
        m = re.search(pattern, cap.text)
        assert m, cap.text
        out = out or [[] for _ in m.groups()]
        for k, v in enumerate(m.groups()):
            out[k].append(float(v))
    return out


def flagged(L, torch, chk):
    """the flagged pairs of a verdict tensor: how many raise each flag, and which pairs raise any (the first 32)"""
    flags = chk[:, L.CHK_W_FLAGS]
    by = {name: int(((flags & (1 << k)) != 0).sum()) for k, name in enumerate(L.CHK_NAMES)}
    idx = (flags != 0).nonzero().flatten()
    return {"flagged_pairs": int(idx.numel()), "by_flag": {k: v for k, v in by.items() if v},
            "flagged": {int(i): [n for k, n in enumerate(L.CHK_NAMES) if int(flags[i]) & (1 << k)] for i in idx[:32].cpu()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("check_bench: no GPU")
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first: see generate_pairs_device)
    import wfa_amd as w
    from wfa_amd import _lib as L
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
    assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
    blob, q_off, q_len, t_off, t_len = d = w.generate_pairs_device(al, 3, args.pairs, 1000, 0.05)
    with StderrCapture():
        rec, ops = al.align_tensors(*d)
    n = rec.shape[0]
    chk = torch.empty((n, L.CHK_WORDS), dtype=torch.int32, device=rec.device)
    passed = torch.empty(n, dtype=torch.int32, device=rec.device)
    os.environ["WFAHIP_DEBUG_TIMING"] = "1"
    # ---- bytes: the check, then the text entry's three passes on the same input
    with StderrCapture():
        _, _, n_flagged = al.check_tensors(rec, ops, *d, out=(chk, passed))  # the warm-up
    (ms,) = timed(args.steps, lambda: al.check_tensors(rec, ops, *d, out=(chk, passed)), r"check alignments: .*kernel ([\d.]+) ms")
    out = {"part": "bytes", "pairs": n, "steps": args.steps, **clock(al, L), "check_kernel_ms": med(ms), "check_kernel_ms_all": ms,
           "n_flagged": n_flagged, **flagged(L, torch, chk)}
    with StderrCapture():
        _, aside, _ = al.check_tensors(rec, ops, *d, mask=L.CHK_NO_ROWS)
    rec_text = rec.clone()
    rec_text[:, L.REC_STATUS] = aside
    with StderrCapture():
        rows = al.alignment_text_tensors(rec_text, ops, *d)  # the warm-up, and the buffers of the timed calls
    ln, scan, wr = timed(args.steps, lambda: al.alignment_text_tensors(rec_text, ops, *d, out=rows),
                         r"alignment text: .*len ([\d.]+) ms, scan ([\d.]+) ms, write ([\d.]+) ms")
    three = [round(a + b + c, 4) for a, b, c in zip(ln, scan, wr)]
    out.update({"text_three_passes_ms": med(three), "text_three_passes_ms_all": three, "text_len_ms": med(ln), "text_scan_ms": med(scan),
                "text_write_ms": med(wr), "text_row_bytes": int(rows[3][-1]), "pairs_set_aside": int((aside == L.PAIR_CHECK_FAILED).sum()),
                "check_within_the_bar": med(ms) <= med(three)})
    print(json.dumps(out), flush=True)
    del rows, rec_text
    # ---- words, every second pair flagged
    q_rc = (torch.arange(n, device=blob.device) & 1).to(torch.uint8)
    stored = store_flagged_reversed(torch, blob, q_off, q_len, q_rc)
    packed, q_woff, t_woff = al.pack_tensors(stored, q_off, q_len, t_off, t_len)
    del stored
    with StderrCapture():
        rec_pk, ops_pk = al.align_tensors_packed(packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
        pk = (rec_pk, ops_pk, packed[:-4], q_woff, q_len, t_woff, t_len)
        _, _, n_flagged = al.check_tensors_packed(*pk, q_rc=q_rc, out=(chk, passed))  # the warm-up
    (ms,) = timed(args.steps, lambda: al.check_tensors_packed(*pk, q_rc=q_rc, out=(chk, passed)), r"check alignments packed: .*kernel ([\d.]+) ms")
    print(json.dumps({"part": "words", "pairs": n, "steps": args.steps, "flags_set": int(q_rc.sum()), **clock(al, L), "check_kernel_ms": med(ms),
                      "check_kernel_ms_all": ms, "n_flagged": n_flagged, **flagged(L, torch, chk)}), flush=True)
    w.RecycleAligner(al)


if __name__ == "__main__":
    main()
