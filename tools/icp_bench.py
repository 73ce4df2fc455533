#!/usr/bin/env python3
"""Device time of the ICP post-step (pointdsc_amd.icp.registration_icp, csrc/icp.hip) at the evaluation's shapes.

    python tools/icp_bench.py [--reps 20] [--warmup 5] [--json]

Cases: 1 pair of N = 1000, 1 pair of N = 5000, 32 pairs of N = 5000 (the fixtures' correspondence endpoints src_keypts /
tgt_keypts, init = the reference's final pose perturbed by 1 deg / 2 cm per pair, so that ICP has work to do), and 4
KITTI-scale pairs of N = 12000 (synthetic.make_pair over a 30 m cube, 20 % inliers, init = the ground truth perturbed
likewise).
Every call is timed with device events after warm-up; reported: us per call, us per iteration (call time / the largest
iteration count of the batch: the launch lasts as long as its slowest pair), the mean iteration count, and per iteration the
bytes and fp64 operations the shapes imply (a model, not a counter reading).

    python tools/icp_bench.py --multiway [--reps 20] [--warmup 5] [--json]

times the multiway driver's edge step instead (pointdsc_amd.multiway): the information matrix at 0.07 m
for 1 and 32 pairs of N = 5000 (fixture endpoints at the reference's pose) and 1 pair of N = 20000 (synthetic.make_pair, 30 %
inliers, at the ground truth), voxel down-sampling of the dense box-room cloud at the three scales, and local_refinement
(three scales of down-sampling + ICP, then the information matrix) of that cloud against a second view of it.
"""
import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from pointdsc_amd import harness, multiway, registration_icp, synthetic  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


def _rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def perturbed(T, deg, cm, rs):
    D = np.eye(4)
    D[:3, :3] = _rot(rs.standard_normal(3), deg)
    d = rs.standard_normal(3)
    D[:3, 3] = d / np.linalg.norm(d) * cm / 100.0
    return (D @ np.asarray(T, np.float64)).astype(np.float32)


def case(fixture, pose_key, bs, seed):
    d = np.load(GOLDEN / fixture)
    return _batch(d["src_keypts"], d["tgt_keypts"], d[pose_key], bs, seed)


def kitti_case(bs, n, seed):
    ps = [synthetic.make_pair(n, inlier_ratio=0.2, noise=0.05, scale=30.0, seed=seed + b) for b in range(bs)]
    return _batch(np.concatenate([p["src_keypts"].numpy() for p in ps]), np.concatenate([p["tgt_keypts"].numpy() for p in ps]),
                  np.concatenate([p["gt_trans"].numpy() for p in ps]), bs, seed)


def _batch(src, tgt, T, bs, seed):
    rs = np.random.RandomState(seed)
    idx = [b % src.shape[0] for b in range(bs)]
    init = np.stack([perturbed(T[i % T.shape[0]], 1.0, 2.0, rs) for i in idx])
    return np.ascontiguousarray(src[idx]), np.ascontiguousarray(tgt[idx]), init


def per_iteration_model(ns, nt, ncorr_mean, cand_mean):
    """Bytes and fp64 operations of one iteration (two passes over the source) per pair, from the shapes: pass 1 reads and
    writes P (48 B), writes corr (4 B), reads 27 x 2 cell bounds (216 B) and every candidate target (16 B each); pass 2 reads
    corr, and P + the target of each correspondence.  fp64: 24 to transform a point, 8 per candidate distance, 7 sums per
    correspondence; 6 + 18 per correspondence for the covariance."""
    bytes_ = ns * (48 + 4 + 216 + 16 * cand_mean) + ns * 4 + ncorr_mean * (24 + 16)
    flops = ns * (24 + 8 * cand_mean) + ncorr_mean * 7 + ncorr_mean * (6 + 18)
    return bytes_, flops


def bench(name, src, tgt, init, reps, warmup):
    dev = torch.device("cuda:0")
    S, Q, I = (torch.from_numpy(x).to(dev) for x in (src, tgt, init))
    for _ in range(warmup):
        res = registration_icp(S, Q, I)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        res = registration_icp(S, Q, I)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    iters = res["iterations"].cpu().numpy()
    ncorr = res["num_correspondences"].cpu().numpy()
    bs, ns = src.shape[0], src.shape[1]
    # candidates per query: targets within the 27 cells (width ~r) around a source point, estimated on the first pair
    P = torch.from_numpy(src[0]).double()
    R, t = torch.from_numpy(init[0][:3, :3]).double(), torch.from_numpy(init[0][:3, 3]).double()
    P = P @ R.T + t
    Qd = torch.from_numpy(tgt[0]).double()
    w = 0.10 * (1 + 1e-3)
    cand = 0.0
    for s in range(0, ns, 1024):
        dd = (P[s:s + 1024, None, :] - Qd[None]).abs()
        cand += float((dd < 1.5 * w).all(-1).sum())          # expected count inside a 3w cube around the point
    cand /= ns
    b_it, f_it = per_iteration_model(ns, tgt.shape[1], float(ncorr.mean()), cand)
    return {"case": name, "pairs": bs, "N": ns, "us_per_call": us, "us_per_iteration": us / max(1, int(iters.max())),
            "mean_iterations": float(iters.mean()), "max_iterations": int(iters.max()),
            "mean_correspondences": float(ncorr.mean()), "candidates_per_query_est": cand,
            "bytes_per_iteration": b_it * bs, "fp64_ops_per_iteration": f_it * bs}


def _time(fn, reps, warmup):
    """us per call of fn() by device events after warm-up."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3, out


def multiway_rows(reps, warmup):
    dev = torch.device("cuda:0")
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    rows = []
    d = np.load(GOLDEN / "n5000_s5.npz")
    big = synthetic.make_pair(20000, inlier_ratio=0.3, noise=0.01, seed=7)
    for name, S, Q, T in (("information 1 x N=5000", d["src_keypts"], d["tgt_keypts"], d["ref_final_trans"]),
                          ("information 32 x N=5000", np.repeat(d["src_keypts"], 32, 0), np.repeat(d["tgt_keypts"], 32, 0),
                           np.repeat(d["ref_final_trans"], 32, 0)),
                          ("information 1 x N=20000", big["src_keypts"].numpy(), big["tgt_keypts"].numpy(), big["gt_trans"].numpy())):
        Sd, Qd, Td = g(S), g(Q), g(T)
        us, out = _time(lambda: multiway.information_matrix(Sd, Qd, multiway.EDGE_DISTANCE, Td), reps, warmup)
        rows.append({"case": name, "us_per_call": us, "mean_correspondences": float(out["num_correspondences"].float().mean())})
    room = synthetic.box_room()
    view, G, _ = harness.second_view(room, 6)
    Rd, Vd = g(room)[None], g(view)[None]
    for v in multiway.VOXEL_SIZES:
        us, out = _time(lambda: multiway.voxel_down_sample(Rd, v), reps, warmup)
        rows.append({"case": f"voxel_down_sample {len(room)} points at {v} m", "us_per_call": us, "points_out": int(out[1][0])})
    init = g(perturbed(G, 2.0, 5.0, np.random.RandomState(106)))[None]
    us, out = _time(lambda: multiway.multi_scale_icp(Rd, Vd, trans=init), max(2, reps // 4), min(warmup, 2))
    rows.append({"case": f"local_refinement {len(room)} x {len(view)} points", "us_per_call": us,
                 "iterations": [int(s["iterations"][0]) for s in out["scales"]],
                 "points": [[int(s["source_counts"][0]), int(s["target_counts"][0])] for s in out["scales"]],
                 "mean_correspondences": float(out["num_correspondences"][0])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--multiway", action="store_true", help="time the multiway edge step (information matrix, voxel down-sampling, local_refinement)")
    a = ap.parse_args()
    if a.multiway:
        rows = multiway_rows(a.reps, a.warmup)
        if a.json:
            print(json.dumps(rows))
            return
        for r in rows:
            print(f"{r['case']:>48s}: {r['us_per_call']:10.1f} us/call  " +
                  "  ".join(f"{k} {v}" for k, v in r.items() if k not in ("case", "us_per_call")))
        return
    cases = [("1 x N=1000", *case("n1000_s1.npz", "ref_final_trans", 1, 1)),
             ("1 x N=5000", *case("n5000_s5.npz", "ref_final_trans", 1, 2)),
             ("32 x N=5000", *case("n5000_s5.npz", "ref_final_trans", 32, 3)),
             ("4 x N=12000 (KITTI)", *kitti_case(4, 12000, 4))]
    rows = [bench(n, s, t, i, a.reps, a.warmup) for n, s, t, i in cases]
    if a.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print(f"{r['case']:>22s}: {r['us_per_call']:9.1f} us/call  {r['us_per_iteration']:7.1f} us/iter  "
              f"iters mean {r['mean_iterations']:5.2f} max {r['max_iterations']:2d}  corr {r['mean_correspondences']:8.1f}  "
              f"cand/query ~{r['candidates_per_query_est']:.1f}  {r['bytes_per_iteration'] / 1e6:.2f} MB/iter  "
              f"{r['fp64_ops_per_iteration'] / 1e6:.2f} Mflop64/iter")


if __name__ == "__main__":
    main()
