#!/usr/bin/env python3
"""Per-stage time of correspondence RANSAC on the device (pointdsc_amd.ransac.ransac_correspondence, csrc/ransac.hip).

    python tools/ransac_bench.py [--reps 5] [--json]

Cases: 1 and 32 pairs of N = 5000 correspondences (synthetic.make_pair, inlier ratio 0.2, seeds 0 ..) at
  baseline   ransac_n 4, I = 1000, every correspondence a candidate          (baseline_3DMatch.py --method RANSAC)
  solver     ransac_n 3, I = 5000, a random mask that keeps about 20 %       (test_3DMatch.py --solver RANSAC on the model's inliers)
all at threshold 0.10.  Stage times are event times on the stream (pdsc_ransac_correspondence_stages): compact | hypothesise | score |
select; the fastest of --reps calls after one warm-up call is printed, next to the time of the whole call between two events around
the plain entry.  The scoring loop's rate is I * M * OPS_PER_POINT fp64 vector instructions over the score stage's time, M being
the pairs' candidate counts; OPS_PER_POINT counts the shipped loop body (ransac_d2 and the two accumulations in csrc/ransac.hip): 11
fused multiply-adds, 1 multiply, 3 subtractions, 1 comparison, 1 addition -- a fused multiply-add counted once.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from pointdsc_amd import ransac_correspondence, synthetic  # noqa: E402

OPS_PER_POINT = 17
N = 5000
CASES = [("baseline", 1, 4, 1000, None), ("baseline", 32, 4, 1000, None), ("solver", 1, 3, 5000, 0.2), ("solver", 32, 3, 5000, 0.2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rows = []
    for name, bs, n, I, share in CASES:
        b = synthetic.make_batch(bs, N, seed=0, inlier_ratio=0.2)
        src, tgt = b["src_keypts"].cuda(), b["tgt_keypts"].cuda()
        mask = None if share is None else torch.from_numpy((np.random.RandomState(1).random_sample((bs, N)) < share).astype(np.float32)).cuda()
        kw = dict(max_correspondence_distance=0.10, ransac_n=n, max_iteration=I, mask=mask, seed=0)
        ransac_correspondence(src, tgt, **kw)                     # warm-up (code objects, allocator)
        torch.cuda.synchronize()
        best, call_us = None, None
        for _ in range(max(1, a.reps)):
            _, labels, info = ransac_correspondence(src, tgt, return_info="stages", **kw)
            if best is None or sum(info["stage_ms"]) < sum(best["stage_ms"]):
                best = info
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ransac_correspondence(src, tgt, **kw)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3
            call_us = us if call_us is None else min(call_us, us)
        m_total = int(best["num_candidates"].sum())
        ops = float(I) * m_total * OPS_PER_POINT
        true_pos = float((torch.stack(list(labels)) * b["gt_labels"].cuda()).sum() / bs)
        rows.append({"case": name, "pairs": bs, "N": N, "ransac_n": n, "I": I, "mean_M": m_total / bs,
                     "stage_us": [round(x * 1e3, 2) for x in best["stage_ms"]], "stages_total_us": round(sum(best["stage_ms"]) * 1e3, 2),
                     "call_us": round(call_us, 2), "score_fp64_Gops": round(ops / (best["stage_ms"][2] * 1e-3) / 1e9, 1),
                     "won": int((best["best_iter"] >= 0).sum()), "mean_true_inliers_labelled": round(true_pos, 1)})
    if a.json:
        print(json.dumps(rows))
        return
    print(f"N {N}, threshold 0.10; times in us (fastest of {a.reps}); rate = I * M * {OPS_PER_POINT} fp64 instructions / score time")
    print(f"{'case':>8s} {'pairs':>5s} {'n':>2s} {'I':>5s} {'mean M':>7s} {'compact':>8s} {'hypoth':>8s} {'score':>9s} {'select':>8s} {'stages':>9s} "
          f"{'call':>9s} {'Gop/s':>8s} {'won':>4s} {'true inl':>8s}")
    for r in rows:
        s = r["stage_us"]
        print(f"{r['case']:>8s} {r['pairs']:5d} {r['ransac_n']:2d} {r['I']:5d} {r['mean_M']:7.0f} {s[0]:8.1f} {s[1]:8.1f} {s[2]:9.1f} {s[3]:8.1f} "
              f"{r['stages_total_us']:9.1f} {r['call_us']:9.1f} {r['score_fp64_Gops']:8.1f} {r['won']:4d} {r['mean_true_inliers_labelled']:8.1f}")


if __name__ == "__main__":
    main()
