#!/usr/bin/env python3
"""The reference's evaluation loop / demo around pointdsc_amd.PointDSC (pointdsc_amd/harness.py).

    python tools/eval_harness.py [--pcd1 a.ply] [--num-pairs 8] [--descriptor {standin,fpfh}] [--snapshot model_best.pkl] [--use-icp]
    python tools/eval_harness.py --pcd1 a.ply --pcd2 b.ply --descriptor fpfh [--use-icp]
    python tools/eval_harness.py --multiway [--num-views 5] [--descriptor {standin,fpfh}] [--batch-pairs 32] [--time 10]
    python tools/eval_harness.py --multiway --posegraph [--use-icp] [--num-views 5]
    python tools/eval_harness.py --baseline {SM,PMC,RANSAC} [--num-pairs 8] [--max-iteration 1000]
    python tools/eval_harness.py --solver RANSAC [--use-icp]

Without --pcd1 the down-sampled demo cloud of tests/golden/demo_clouds_vox005.npz (reference demo_data/cloud_bin_0.ply at
0.05 m) is used.  Every pair = the cloud against a seeded second view of it (partial overlap, noise, random rigid motion),
stand-in descriptors with a known outlier share (--descriptor standin, the default) or the device's FPFH of each view
(--descriptor fpfh: misc/cal_fpfh.py:21-26 on the GPU, pointdsc_amd.features), GPU correspondence construction, forward,
device-side stats row.  --pcd2 registers the real second cloud instead (the demo's own pair, demo_registration.py:101-117, always
with FPFH): there is no ground truth, so the pose and the inlier count are printed only.
--multiway runs the multiway driver's pairwise loop instead (multiway/test_multi_ate.py:98-157, harness.multiway_edges): every pair
of --num-views seeded views of the cloud; adjacent views through multi-scale ICP (certain edges), the others through the forward,
the device-side information matrix and the overlap gate (uncertain edges); prints the edges a pose graph would receive.
--multiway --posegraph goes on as the driver does (:159-227, harness.multiway_trajectory): node chain, pose-graph optimisation on the
device (with --use-icp: multi-scale ICP of every edge and a second optimisation), and the driver's lines -- "Before optimization ...
nodes ... edges", "After optimization ...", "Mean Absolute Trajectory Error: ... cm" against the views' true poses.
--baseline runs a classical baseline of baseline_scripts/baseline_3DMatch.py (--method SM / PMC / RANSAC: pointdsc_amd.baselines) in
place of the model on the same pairs and prints the same stats rows.  --solver RANSAC is evaluation/test_3DMatch.py's: the model's
pose and labels are replaced by correspondence RANSAC over the correspondences it labelled as inliers (pointdsc_amd.ransac).
Registration Recall on 3DMatch-FCGF itself needs the released weights and the dataset (both absent here): pass
--snapshot / real descriptors when they exist; the loop is the same.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from pointdsc_amd import PointDSC, harness, workloads  # noqa: E402


def multiway(model, cloud, a):
    views = harness.demo_views(cloud, a.num_views, corrupt=min(a.outlier_share, 0.4), descriptor=a.descriptor, voxel=a.voxel)
    if a.posegraph:
        return posegraph(model, views, a)
    edges = harness.multiway_edges(model, views, use_mutual=a.mutual, batch_pairs=a.batch_pairs)
    if a.time > 0:                            # the pass above was the warm-up
        ms = []
        for _ in range(a.time):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            harness.multiway_edges(model, views, use_mutual=a.mutual, batch_pairs=a.batch_pairs)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        print(f"multiway_edges views={a.num_views} batch_pairs={a.batch_pairs} mutual={a.mutual}: median {np.median(ms):.2f} ms "
              f"(min {min(ms):.2f} max {max(ms):.2f}, {a.time} rounds)")
    if a.json:
        print(json.dumps({"edges": [{"source": s, "target": t, "transformation": T.tolist(), "information": info.tolist(),
                                     "uncertain": bool(u)} for s, t, T, info, u in edges]}))
        return
    pairs = a.num_views * (a.num_views - 1) // 2
    print(f"{len(cloud)} points, {a.num_views} views, {pairs} pairs -> {len(edges)} edges ({pairs - len(edges)} dropped by the overlap gate)")
    for s, t, T, info, u in edges:
        gt = views[t]["pose"] @ np.linalg.inv(views[s]["pose"])
        d = T @ np.linalg.inv(gt)
        re = np.degrees(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1)))
        print(f"{s:3d} -> {t:3d}  {'uncertain' if u else 'certain  '}  correspondences {info[5, 5]:7.0f}  RE {re:7.3f} deg  "
              f"TE {np.linalg.norm(T[:3, 3] - gt[:3, 3]) * 100:7.3f} cm")


def posegraph(model, views, a):
    """multiway/test_multi_ate.py:164, :175 (:215, :225 with --use-icp) and :268."""
    res = harness.multiway_trajectory(model, views, use_icp=a.use_icp, use_mutual=a.mutual, batch_pairs=a.batch_pairs)
    records = [res["first_record"].cpu().numpy()] if a.use_icp else []
    records.append(res["record"].cpu().numpy())
    if a.json:
        print(json.dumps({"ate_cm": res["ate_cm"], "errors_cm": res["errors_cm"].cpu().tolist(), "nodes": res["nodes"].cpu().tolist(),
                          "keep": res["keep"].cpu().tolist(), "records": [r.tolist() for r in records]}))
        return
    for i, r in enumerate(records):
        if i:
            print("Refine each edge with ICP ...")
        print(f"Before optimization {len(views)} nodes {int(r[9])} edges")
        print("Optimizing PoseGraph ...")
        print(f"  pass 1: {int(r[1])} iterations, {int(r[2])} solves, objective {r[3]:.6g}; pass 2: {int(r[5])} iterations, {int(r[6])} solves, "
              f"objective {r[7]:.6g}" + ("  (INVALID GRAPH)" if r[0] else ""))
        print(f"After optimization {len(views)} nodes {int(r[11])} edges")
    print(f"Mean Absolute Trajectory Error: {res['ate_cm']:.2f} cm")


def real_pair(model, cloud, a):
    """demo_registration.py:101-117 on two real clouds: FPFH -> matching -> forward (-> ICP); no ground truth."""
    from pointdsc_amd import icp_refine
    from pointdsc_amd.correspondences import build_correspondences
    dev = torch.device("cuda:0")
    with torch.no_grad():
        if a.fpfh_recipe == "demo":             # demo_registration.py:37-44: the raw vertices go to the device, nothing is down-sampled here
            cloud2 = harness.read_ply_xyz(a.pcd2)
            pts, desc = zip(*(harness.device_demo_fpfh(c, a.voxel) for c in (cloud, cloud2)))
            cloud, cloud2 = pts
        else:
            cloud2 = harness.voxel_down_sample(harness.read_ply_xyz(a.pcd2), a.voxel)
            pts = [torch.from_numpy(c).to(dev) for c in (cloud, cloud2)]
            desc = [harness.device_fpfh(c, a.voxel) for c in (cloud, cloud2)]
        c = build_correspondences(desc[0], desc[1], pts[0], pts[1], use_mutual=a.mutual)
        res = model({"corr_pos": c["corr_pos"], "src_keypts": c["src_keypts"], "tgt_keypts": c["tgt_keypts"], "testing": True})
        trans = res["final_trans"]
        if a.use_icp:
            trans = icp_refine(c["src_keypts"], c["tgt_keypts"], trans, a.icp_distance)
        T, inliers = trans[0].cpu().numpy(), int((res["final_labels"][0] > 0).sum())
    if a.json:
        print(json.dumps({"points": [len(cloud), len(cloud2)], "correspondences": int(c["corr_pos"].shape[1]), "inliers": inliers,
                          "transformation": T.tolist()}))
        return
    print(f"{len(cloud)} / {len(cloud2)} points after {a.voxel} m voxel down-sampling; {c['corr_pos'].shape[1]} correspondences, "
          f"{inliers} predicted inliers" + (" (ICP post-step)" if a.use_icp else ""))
    print(np.array2string(T, precision=6, suppress_small=True))


def validate(a):
    from pointdsc_amd import synthetic
    kw = dict(workloads.BASE_MODEL)
    model = PointDSC(**kw)
    if a.snapshot:
        print(model.load_state_dict(torch.load(a.snapshot, map_location="cpu"), strict=False))
    else:
        model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    model = model.eval().cuda()
    batches = [synthetic.make_batch(16, 1000, seed=100 + 16 * i, inlier_ratio=0.3) for i in range(a.num_batches)]
    means = harness.validate(model, batches)
    if a.json:
        print(json.dumps(means))
        return
    print(f"{a.num_batches} synthetic batches of 16 pairs x 1000 correspondences")
    for k, v in means.items():
        print(f"{k}: {v:.6f}")


def train(a):
    """--train: a few optimiser steps of harness.train_epoch on the synthetic batches --validate uses; the validation meters of
    the same batches before and after."""
    from pointdsc_amd import TrainablePointDSC, synthetic
    model = TrainablePointDSC(**dict(workloads.BASE_MODEL), differentiable_trans=a.weight_transformation > 0, fused_layers=a.fused_layers,
                              fused_linears=a.fused_linears)
    if a.snapshot:
        print(model.load_state_dict(torch.load(a.snapshot, map_location="cpu"), strict=False))
    else:
        model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    model = model.cuda()
    batches = [synthetic.make_batch(16, 1000, seed=100 + 16 * i, inlier_ratio=0.3) for i in range(a.num_batches)]
    # config.py:48-53 and train_3DMatch.py:48-66: ADAM (the default) or SGD with momentum 0.9, weight decay 1e-6
    if a.device_optimizer:          # guard, update and skip decision on the device: train_epoch reads nothing back in its loop
        from pointdsc_amd import DeviceAdam, DeviceSGD
        optimizer = (DeviceAdam(model.parameters(), lr=a.lr, weight_decay=1e-6) if a.optimizer == "adam" else
                     DeviceSGD(model.parameters(), lr=a.lr, momentum=0.9, weight_decay=1e-6))
    elif a.optimizer == "adam":
        optimizer = torch.optim.Adam(model.parameters(), lr=a.lr, weight_decay=1e-6)
    else:
        optimizer = torch.optim.SGD(model.parameters(), lr=a.lr, momentum=0.9, weight_decay=1e-6)
    before = harness.validate(model.eval(), batches)
    steps = [batches[i % len(batches)] for i in range(a.train_steps)]
    meters = harness.train_epoch(model.train(), steps, optimizer, weights=(1.0, 1.0, a.weight_transformation))
    after = harness.validate(model.eval(), batches)
    if a.json:
        print(json.dumps({"before": before, "train": meters, "after": after}))
        return
    name = ("Device" if a.device_optimizer else "") + {"adam": "Adam", "sgd": "SGD"}[a.optimizer]
    print(f"{a.train_steps} {name} steps (lr {a.lr}) over {a.num_batches} synthetic batches of 16 pairs x 1000 correspondences; "
          f"{meters['skipped']} skipped; weighted loss {meters['loss_first']:.6f} -> {meters['loss_last']:.6f}")
    print(f"{'meter':18s} {'validation before':>18s} {'training mean':>18s} {'validation after':>18s}")
    for k in harness.VALIDATE_NAMES:
        print(f"{k:18s} {before[k]:18.6f} {meters[k]:18.6f} {after[k]:18.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pcd1", default=None, help="PLY file (binary LE / ascii, float xyz); default: the demo fixture")
    ap.add_argument("--pcd2", default=None, help="PLY file of the real second cloud: register --pcd1 onto it with FPFH descriptors "
                    "(no ground truth: pose and inlier count only)")
    ap.add_argument("--descriptor", choices=("standin", "fpfh"), default="standin",
                    help="stand-in descriptors with a known outlier share, or FPFH on the device (misc/cal_fpfh.py:21-26)")
    ap.add_argument("--fpfh-recipe", choices=("cal_fpfh", "demo"), default="cal_fpfh",
                    help="with --pcd1 / --pcd2: cal_fpfh = down-sample on the host, then normals and FPFH on the device (misc/cal_fpfh.py); "
                    "demo = demo_registration.py:37-44 on the device from the raw vertices (normals on the raw cloud, voxel step that "
                    "averages them, FPFH)")
    ap.add_argument("--voxel", type=float, default=0.05, help="config.downsample of the 3DMatch snapshot")
    ap.add_argument("--num-pairs", type=int, default=8)
    ap.add_argument("--outlier-share", type=float, default=0.6, help="share of stand-in descriptors replaced by noise")
    ap.add_argument("--snapshot", default=None, help="released model_best.pkl (load_state_dict(strict=False)); default: seeded weights")
    ap.add_argument("--mutual", action="store_true", help="mutual nearest neighbours only (datasets/ThreeDMatch.py:286-288)")
    ap.add_argument("--batch-size", type=int, default=1, help="pairs per (ragged) model call; the reference evaluates one pair per call")
    ap.add_argument("--use-icp", action="store_true", help="refine every pose by point-to-point ICP on the device (test_3DMatch.py --use_icp)")
    ap.add_argument("--icp-distance", type=float, default=0.10, help="max_correspondence_distance of the ICP post-step")
    ap.add_argument("--multiway", action="store_true", help="the multiway driver's edge loop over --num-views views (test_multi_ate.py:98-157)")
    ap.add_argument("--num-views", type=int, default=5)
    ap.add_argument("--batch-pairs", type=int, default=1, help="with --multiway: loop-closure candidates per batched correspondence "
                    "construction and ragged forward (harness.multiway_edges batch_pairs); 1 = one pair per call")
    ap.add_argument("--time", type=int, default=0, help="with --multiway: repeat the edge loop this many times after the first pass and "
                    "print the median wall time")
    ap.add_argument("--posegraph", action="store_true", help="with --multiway: node chain, pose-graph optimisation on the device and the ATE "
                    "(test_multi_ate.py:159-227, :268); --use-icp adds the ICP refinement of the edges and the second optimisation")
    ap.add_argument("--baseline", choices=harness.BaselineModel.METHODS + ("RANSAC",), default=None,
                    help="run this baseline of baseline_3DMatch.py in place of the model (pair loop only)")
    ap.add_argument("--max-iteration", type=int, default=1000, help="with --baseline RANSAC: hypotheses per pair (baseline_3DMatch.py:131)")
    ap.add_argument("--solver", choices=harness.SOLVERS, default="SVD", help="test_3DMatch.py --solver: RANSAC replaces every pose and "
                    "label set by correspondence RANSAC (ransac_n 3, 5000 iterations) over the model's inliers, on the device")
    ap.add_argument("--validate", action="store_true", help="the validation loop of libs/trainer.py:158-222 on the device "
                    "(harness.validate: validation forward + the three losses) over --num-batches synthetic batches (bs 16, N 1000)")
    ap.add_argument("--num-batches", type=int, default=4, help="with --validate: batches of 16 pairs")
    ap.add_argument("--train", action="store_true", help="the training loop of libs/trainer.py:79-136 on the device (harness.train_epoch on a "
                    "TrainablePointDSC: train()-mode forward, classification + spectral-matching loss, backward, Adam) for --train-steps "
                    "steps over the --num-batches synthetic batches of --validate, with the validation meters before and after")
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--lr", type=float, default=1e-4, help="with --train (config.py:52)")
    ap.add_argument("--weight-transformation", type=float, default=0.0, help="with --train: config.py:43, the weight of the transformation "
                    "loss in the objective; above 0 the model is built with differentiable_trans=True")
    ap.add_argument("--optimizer", choices=("adam", "sgd"), default="adam", help="with --train (train_3DMatch.py:48-66)")
    ap.add_argument("--device-optimizer", action="store_true", help="with --train: pointdsc_amd.DeviceAdam / DeviceSGD instead of "
                    "torch.optim's: finite-gradient guard, update and skip decision on the device (DESIGN.md section 8 f-25)")
    ap.add_argument("--fused-layers", action="store_true", help="with --train: the blocks' conv + batch-norm + ReLU groups as device kernels "
                    "(TrainablePointDSC(fused_layers=True), pointdsc_amd.conv_bn_relu)")
    ap.add_argument("--fused-linears", action="store_true", help="with --train: layer0, the q|k|v projections, fc_message.6 with its residual "
                    "and the classification head as device kernels (TrainablePointDSC(fused_linears=True): pointdsc_amd.linear_rows, "
                    "qkv_projection, classification_head)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.train:
        if a.validate or a.baseline or a.pcd1 or a.pcd2 or a.multiway or a.posegraph:
            ap.error("--train runs the model on synthetic batches: not with --validate, --baseline, --pcd1, --pcd2, --multiway or --posegraph")
        return train(a)
    if a.validate:
        if a.baseline or a.pcd1 or a.pcd2 or a.multiway or a.posegraph:
            ap.error("--validate runs the model on synthetic batches: not with --baseline, --pcd1, --pcd2, --multiway or --posegraph")
        return validate(a)
    if a.baseline and (a.pcd2 or a.multiway or a.posegraph or a.snapshot):
        ap.error("--baseline replaces the model in the pair loop: not with --pcd2, --multiway, --posegraph or --snapshot")
    if a.fpfh_recipe == "demo" and not (a.pcd1 and a.pcd2):
        ap.error("--fpfh-recipe demo goes with --pcd1 and --pcd2")
    if a.pcd1 and a.fpfh_recipe == "demo":
        cloud = harness.read_ply_xyz(a.pcd1)              # raw: real_pair sends it to the device as it is
    elif a.pcd1:
        cloud = harness.voxel_down_sample(harness.read_ply_xyz(a.pcd1), a.voxel)
    else:
        cloud = np.load(ROOT / "tests" / "golden" / "demo_clouds_vox005.npz")["cloud_bin_0"]
    kw = dict(workloads.BASE_MODEL)                       # evaluation/test_3DMatch.py:215-224 with the snapshot's config.json
    if a.baseline == "RANSAC":
        model = harness.RansacModel(kw["inlier_threshold"], max_iteration=a.max_iteration)
    elif a.baseline:
        model = harness.BaselineModel(a.baseline, kw["inlier_threshold"])
    else:
        model = PointDSC(**kw)
        if a.snapshot:
            print(model.load_state_dict(torch.load(a.snapshot, map_location="cpu"), strict=False))      # test_3DMatch.py:225-226
        else:
            model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
        model = model.eval().cuda()
    if a.pcd2:
        if not a.pcd1:
            ap.error("--pcd2 goes with --pcd1")
        return real_pair(model, cloud, a)
    if a.posegraph and not a.multiway:
        ap.error("--posegraph goes with --multiway")
    if a.multiway:
        return multiway(model, cloud, a)
    pairs = harness.demo_pairs(cloud, a.num_pairs, corrupt=a.outlier_share, descriptor=a.descriptor, voxel=a.voxel)
    stats = harness.eval_scene(model, pairs, scene_ind=0,
                               inlier_threshold=kw["inlier_threshold"], use_mutual=a.mutual, batch_size=a.batch_size,
                               use_icp=a.use_icp, icp_distance=a.icp_distance, solver=a.solver)
    summ = harness.summarize(stats)
    if a.json:
        print(json.dumps({"stats_columns": harness.STATS_NAMES, "stats": stats.tolist(), "summary": summ}))
        return
    print(f"{len(cloud)} points after {a.voxel} m voxel down-sampling; {a.num_pairs} pairs" + (" (ICP post-step)" if a.use_icp else "") +
          (f" (baseline {a.baseline})" if a.baseline else "") + (" (solver RANSAC)" if a.solver == "RANSAC" else ""))
    print(" ".join(f"{n[:10]:>10s}" for n in harness.STATS_NAMES))
    for row in stats:
        print(" ".join(f"{v:10.4f}" for v in row))
    for k, v in summ.items():
        print(f"{k}: {v:.4f}" if isinstance(v, float) else f"{k}: {v}")


if __name__ == "__main__":
    main()
