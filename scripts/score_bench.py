"""Score-only against full alignment on the same host inputs, in one process (include/wfa_hip.h: wfahip_score_batch vs
wfahip_align_batch).  Workloads as bench.py generates them: c3 = 1e6 x 1 kbp @5 %, seed 3, global, wf-adaptive 10/50/1,
penalties 4/6/2; g3 = the same pairs semi-global.  After a warm-up of each entry, the two calls alternate --steps times;
per entry: pairs/s, wall ms per call (host clock around the synchronous call) and the kernel ms last_timing reports.
The scores of the two entries must agree.  One JSON line per workload.

    python scripts/score_bench.py [--configs c3,g3] [--pairs 1000000] [--steps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c3": True, "g3": False}  # name: global alignment


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,g3")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU")
    import wfa_amd as w
    arrays = w.generate_pairs(3, args.pairs, 1000, 0.05, n_threads=16)
    for name in args.configs.split(","):
        al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=CONFIGS[name]), device=0)
        assert al.AdaptiveReduction(w.DefaultAdaptiveOption) is None
        full = lambda: al.align_arrays(*arrays)
        score = lambda: al.score_arrays(*arrays)
        full(), score()  # warm-up: buffers, code objects
        legs = {"align": [], "score": []}
        ref = got = None
        for _ in range(args.steps):
            for leg, fn in (("align", full), ("score", score)):
                t0 = time.perf_counter()
                r = fn()
                dt = (time.perf_counter() - t0) * 1e3
                t = al.last_timing()
                legs[leg].append((dt, t.kernel_ms, t.main_kernel_kind, t.n_retried_pairs, t.arena_bytes))
                if leg == "align":
                    ref = r
                else:
                    got = r
        st, sc = got
        assert np.array_equal(st, ref.status) and np.array_equal(sc, np.where(ref.status == 0, ref.score, 0)), name
        out = {"config": name, "pairs": args.pairs, "steps": args.steps}
        for leg, v in legs.items():
            wall = float(np.median([x[0] for x in v]))
            out[leg] = {"pairs_per_s": args.pairs / wall * 1e3, "wall_ms": wall, "kernel_ms": float(np.median([x[1] for x in v])),
                        "main_kernel_kind": v[-1][2], "n_retried_pairs": v[-1][3], "arena_bytes": v[-1][4],
                        "wall_ms_all": [round(x[0], 2) for x in v]}
        out["scores_equal"] = True
        print(json.dumps(out), flush=True)
        w.RecycleAligner(al)


if __name__ == "__main__":
    main()
