"""The display rows from packed words (KERNELS.md 4t) against the display rows from bytes (4q), in one process on one GPU.  One JSON
line per part.

Workload: the benchmark's headline batch -- 1e6 x 1 kbp @5 % (seed 3, penalties 4/6/2, wf-adaptive 10/50/1, global) -- generated on
the device.  Every second pair is flagged: its query is stored reverse-complemented (on the device, by index arithmetic), so that the
flagged alignment is the alignment of the generated pair.  The stored bytes are packed (wfahip_pack_pairs_device) and aligned once
from the words with the flags (wfahip_align_batch_packed_device); the pairs whose ops overrun a sequence under wf-adaptive are set
aside as scripts/alignment_text_bench.py does.  Then two renderings of the same records and ops are timed, --runs times each,
alternating, full and trimmed:

  packed   wfahip_alignment_text_packed_device over the words, offsets, lengths and flags
  bytes    wfahip_alignment_text_device over the GENERATED blob, which holds the same sequences with the flagged queries
           reverse-complemented -- the strand the records speak of

For each the hipEvent ms of the length kernel, the scan's kernels and the write kernel (the library prints them under
WFAHIP_DEBUG_TIMING=1; this script reads them back from its own stderr) and the wall ms of the call.  The margin of the comparison
is the byte entry's own spread (max - min) over its runs; the rows of the two are compared byte for byte.

    python scripts/alignment_text_packed_bench.py [--pairs 1000000] [--runs 3]
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from alignment_text_bench import set_aside  # noqa: E402
from cigar_text_bench import StderrCapture, clock, med  # noqa: E402

PASSES = ("len", "scan", "write")


def store_flagged_reversed(torch, blob, q_off, q_len, flags, chunk=50_000):
    """a copy of blob in which the query of every flagged pair is replaced by its reverse complement"""
    comp = torch.arange(256, dtype=torch.uint8, device=blob.device)
    for a, b in ((ord("A"), ord("T")), (ord("C"), ord("G"))):
        comp[a], comp[b] = b, a
    out = blob.clone()
    idx = torch.nonzero(flags).flatten()
    for k in range(0, idx.numel(), chunk):
        i = idx[k:k + chunk]
        off, ln = q_off[i], q_len[i].to(torch.int64)
        j = torch.arange(int(ln.max()), dtype=torch.int64, device=blob.device)[None, :]
        live = j < ln[:, None]
        dst = (off[:, None] + j)[live]
        src = (off[:, None] + ln[:, None] - 1 - j)[live]
        out[dst] = comp[blob[src].to(torch.int64)]
    return out


def one_call(torch, render, pattern):
    """(wall ms, {pass: hipEvent ms}) of one rendering"""
    torch.cuda.synchronize()
    with StderrCapture() as cap:
        t0 = time.perf_counter()
        render()
        wall = (time.perf_counter() - t0) * 1e3
    m = re.search(pattern + r": .*len ([\d.]+) ms, scan ([\d.]+) ms, write ([\d.]+) ms", cap.text)
    assert m, cap.text
    return wall, dict(zip(PASSES, (float(v) for v in m.groups())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("alignment_text_packed_bench: no GPU")
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first: see generate_pairs_device)
    import wfa_amd as w
    from wfa_amd import _lib as L
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=True), device=0)
    assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
    blob, q_off, q_len, t_off, t_len = w.generate_pairs_device(al, 3, args.pairs, 1000, 0.05)
    q_rc = (torch.arange(args.pairs, device=blob.device) & 1).to(torch.uint8)
    stored = store_flagged_reversed(torch, blob, q_off, q_len, q_rc)
    packed, q_woff, t_woff = al.pack_tensors(stored, q_off, q_len, t_off, t_len)
    del stored
    with StderrCapture():
        rec, ops = al.align_tensors_packed(packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
    rec, aside = set_aside(al, L, rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc)
    print(json.dumps({"part": "input", "pairs": args.pairs, "flagged": int(q_rc.sum()), "packed_words": int(packed.numel()) - 4,
                      "blob_bytes": int(blob.numel()), "pairs_not_ok": int((rec[:, L.REC_STATUS] != 0).sum()),
                      "pairs_set_aside_because_their_ops_overrun_a_sequence": aside, **clock(al, L)}), flush=True)
    os.environ["WFAHIP_DEBUG_TIMING"] = "1"
    for only in (False, True):
        out_pk = al.alignment_text_tensors_packed(rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc, only_aligned=only)  # the warm-up,
        out_by = al.alignment_text_tensors(rec, ops, blob, q_off, q_len, t_off, t_len, only_aligned=only)                      # and the buffers
        legs = {"packed": (lambda: al.alignment_text_tensors_packed(rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=q_rc,
                                                                   only_aligned=only, out=out_pk), "alignment text packed"),
                "bytes": (lambda: al.alignment_text_tensors(rec, ops, blob, q_off, q_len, t_off, t_len, only_aligned=only, out=out_by),
                          "alignment text")}
        wall = {k: [] for k in legs}
        ev = {k: {p: [] for p in PASSES} for k in legs}
        for _ in range(args.runs):  # alternating
            for k, (render, pattern) in legs.items():
                ms, passes = one_call(torch, render, pattern)
                wall[k].append(round(ms, 4))
                for p in PASSES:
                    ev[k][p].append(passes[p])
        total = int(out_pk[3][-1])
        res = {"part": "trimmed" if only else "full", "runs": args.runs, "row_bytes": total, "row_bytes_per_pair": round(total / args.pairs, 2),
               "rows_equal": bool(all(torch.equal(a, b) for a, b in zip(out_pk, out_by)))}
        three = {k: [round(sum(ev[k][p][r] for p in PASSES), 4) for r in range(args.runs)] for k in legs}
        for k in legs:
            res[k] = {"call_wall_ms": wall[k], **{p + "_ms": ev[k][p] for p in PASSES}, "three_passes_ms": three[k],
                      "write_ms_median": med(ev[k]["write"]), "three_passes_ms_median": med(three[k])}
        for name, a, b in (("write", ev["packed"]["write"], ev["bytes"]["write"]), ("three_passes", three["packed"], three["bytes"])):
            spread = round(max(b) - min(b), 4)
            res[name + "_bytes_spread_ms"] = spread
            res[name + "_packed_minus_bytes_ms"] = round(med(a) - med(b), 4)
            res[name + "_packed_no_slower"] = bool(med(a) <= med(b) + spread)
        print(json.dumps(res), flush=True)
        del out_pk, out_by
    del os.environ["WFAHIP_DEBUG_TIMING"]
    w.RecycleAligner(al)


if __name__ == "__main__":
    main()
