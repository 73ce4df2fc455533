"""Evaluation / demo harness around ``PointDSC.forward`` -- what the reference's callers do on either side of the path.

Replicates, without open3d / easydict (absent here):
  * ``evaluation/test_3DMatch.py:20-103``  eval_3DMatch_scene: per-pair loop, ``model(data)`` under no_grad, the
    12-column stats row (0 success, 1 RE deg, 2 TE cm, 3 input inliers, 4 input inlier ratio, 5 output true positives,
    6 precision, 7 recall, 8 F1, 9 model time, 10 data time, 11 scene index) and the summary lines of
    ``eval_3DMatch`` (:141-176: recall, mean RE / TE over the successful pairs, mean P / R / F1, mean times);
  * ``demo_registration.py:37-44,101-117``  cloud -> voxel down-sampling -> descriptors -> nearest-neighbour matching
    -> ``corr_pos`` -> ``model(data)``.
The arithmetic on the path runs in libpointdsc_hip.so (correspondence construction f-2, forward a-*, stats row f-4, the
optional ICP post-step f-5, the RANSAC solver f-21, the multiway driver's edge step f-6: ``multiway_edges``, its pose-graph optimisation and ATE f-8:
``multiway_trajectory``);
this module is host plumbing: PLY reading (binary little-endian float xyz), open3d-style voxel
down-sampling in numpy, the pair loop, timers (``utils/timer.py`` semantics: wall clock, here with a device
synchronisation so that model time is the GPU's).

Descriptors: FCGF extraction is upstream of the path and needs MinkowskiEngine and a checkpoint (absent).  FPFH runs on the
device (``features.fpfh_descriptors``, f-7: the recipe of misc/cal_fpfh.py:21-26): ``demo_pairs`` / ``demo_views`` compute it with
``descriptor="fpfh"``, so that cloud -> descriptors -> matching -> forward -> ICP runs on real geometry.  Their default,
``standin_descriptors``, provides seeded unit vectors that agree for points that coincide under the ground-truth motion (a
stand-in with a controllable inlier ratio, NOT a feature extractor).  With real descriptors + the released weights the same loop
is the Registration-Recall driver.
"""
from __future__ import annotations

import time
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .correspondences import CorrPool, build_correspondences, build_correspondences_batch
from .features import extract_fpfh_features, fpfh_descriptors
from .icp import icp_refine
from .multiway import local_refinement, loop_closure_edge
from .ransac import ransac_correspondence

STATS_NAMES = ("success", "RE_deg", "TE_cm", "input_inliers", "input_inlier_ratio", "output_true_positives",
               "precision", "recall", "f1", "model_time_s", "data_time_s", "scene_ind")


# ---------------------------------------------------------------------------------------------------------------
# clouds
# ---------------------------------------------------------------------------------------------------------------
def read_ply_xyz(path) -> np.ndarray:
    """Vertices of a PLY file as float32 [n,3] (ascii or binary_little_endian; x, y, z may sit among other properties)."""
    raw = Path(path).read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    fmt, n, props, in_vertex = None, 0, [], False
    np_types = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1", "char": "i1",
                "int8": "i1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
                "uint": "u4", "uint32": "u4"}
    for line in raw[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            in_vertex = tok[1] == "vertex"
            if in_vertex:
                n = int(tok[2])
        elif tok[0] == "property" and in_vertex:
            if tok[1] == "list":
                raise ValueError("list property inside the vertex element")
            props.append((tok[2], np_types[tok[1]]))
    names = [p[0] for p in props]
    if not all(a in names for a in "xyz"):
        raise ValueError(f"{path}: no x/y/z vertex properties")
    if fmt == "binary_little_endian":
        rec = np.frombuffer(raw, dtype=np.dtype([(nm, "<" + ty) for nm, ty in props]), count=n, offset=end)
        return np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
    if fmt == "ascii":
        rows = np.loadtxt(raw[end:].decode().splitlines()[:n], dtype=np.float64, ndmin=2)
        return rows[:, [names.index(a) for a in "xyz"]].astype(np.float32)
    raise ValueError(f"{path}: unsupported PLY format {fmt}")


def voxel_down_sample(points: np.ndarray, voxel: float) -> np.ndarray:
    """open3d ``PointCloud.voxel_down_sample``: voxel grid anchored at min_bound - voxel/2, one output point per occupied
    voxel = the mean of its points (output ordered by voxel index; open3d's order is a hash-map artefact)."""
    pts = np.asarray(points, dtype=np.float64)
    origin = pts.min(axis=0) - 0.5 * voxel
    idx = np.floor((pts - origin) / voxel).astype(np.int64)
    dims = idx.max(axis=0) + 1
    key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    order = np.argsort(key, kind="stable")
    key, pts = key[order], pts[order]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    sums = np.add.reduceat(pts, first, axis=0)
    counts = np.diff(np.r_[first, len(key)])
    return (sums / counts[:, None]).astype(np.float32)


def random_rigid(rs: np.random.RandomState, max_trans: float = 1.0) -> np.ndarray:
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = q
    T[:3, 3] = rs.uniform(-max_trans, max_trans, 3)
    return T


def standin_descriptors(points_in_common_frame: np.ndarray, dim: int, cell: float, seed: int, corrupt: float,
                        rs: np.random.RandomState) -> np.ndarray:
    """Seeded unit descriptors that agree for points falling into the same `cell`-sized cube of the COMMON frame (i.e.
    for true matches) -- a stand-in for FPFH / FCGF with a controllable outlier share (`corrupt` = fraction of points
    whose descriptor is replaced by an unrelated one).  Not a feature extractor: it needs the ground-truth frame."""
    q = np.floor(points_in_common_frame / cell).astype(np.int64)
    h = (q[:, 0] * 73856093) ^ (q[:, 1] * 19349663) ^ (q[:, 2] * 83492791) ^ seed
    out = np.empty((len(q), dim), dtype=np.float32)
    uniq, inv = np.unique(h, return_inverse=True)
    table = np.stack([np.random.RandomState(int(u) & 0x7FFFFFFF).standard_normal(dim) for u in uniq]).astype(np.float32)
    out[:] = table[inv]
    bad = rs.random_sample(len(q)) < corrupt
    out[bad] = rs.standard_normal((int(bad.sum()), dim)).astype(np.float32)
    out += rs.standard_normal(out.shape).astype(np.float32) * 0.05
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def second_view(points: np.ndarray, seed: int, keep: float = 0.7, noise: float = 0.005) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A second 'scan' of the same scene: a random sub-set of the points (partial overlap), sensor noise, moved by a
    random rigid motion.  Returns (tgt_points [m,3], gt_trans [4,4] with p_tgt = R p_src + t, tgt_points_in_src_frame)."""
    rs = np.random.RandomState(seed)
    T = random_rigid(rs)
    sel = rs.random_sample(len(points)) < keep
    in_src = points[sel] + rs.standard_normal((int(sel.sum()), 3)).astype(np.float32) * noise
    tgt = in_src @ T[:3, :3].T + T[:3, 3]
    return tgt.astype(np.float32), T, in_src.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# the pair loop (evaluation/test_3DMatch.py:20-103)
# ---------------------------------------------------------------------------------------------------------------
def gt_labels_from_trans(src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, gt_trans: torch.Tensor, thr: float) -> torch.Tensor:
    """datasets/ThreeDMatch.py:292-296: a correspondence is an inlier if ||R src + t - tgt|| < inlier_threshold."""
    warped = src_keypts @ gt_trans[:3, :3].T + gt_trans[:3, 3]
    return ((warped - tgt_keypts).norm(dim=-1) < thr).float()


class BaselineModel:
    """A classical baseline of baseline_scripts/baseline_3DMatch.py (``--method SM`` / ``PMC``) behind the model's calling
    convention, so that eval_scene runs it in place of the network: data dict with corr_pos / src_keypts / tgt_keypts ([1,N,.]
    tensors, or lists of per-pair [N,.] tensors) -> {"final_trans": [B,4,4], "final_labels": per-pair [N] rows}."""
    METHODS = ("SM", "PMC")

    def __init__(self, method: str, inlier_threshold: float = 0.10):
        if method not in self.METHODS:
            raise ValueError(f"baseline must be one of {self.METHODS}, got {method!r}")
        self.method, self.inlier_threshold = method, float(inlier_threshold)

    def __call__(self, data):
        from . import baselines
        fn = baselines.SM if self.method == "SM" else baselines.PMC
        c, s, t = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
        if torch.is_tensor(c):
            trans, labels = fn(c, s, t, self.inlier_threshold)
            return {"final_trans": trans, "final_labels": labels}
        out = [fn(ci[None], si[None], ti[None], self.inlier_threshold) for ci, si, ti in zip(c, s, t)]      # every pair has its own N
        return {"final_trans": torch.cat([o[0] for o in out]), "final_labels": [o[1][0] for o in out]}


class RansacModel:
    """baseline_scripts/baseline_3DMatch.py ``--method RANSAC`` (:80-98, open3d registration_ransac_based_on_correspondence over all
    correspondences of a pair) behind the calling convention of ``BaselineModel.__call__``: data dict with src_keypts / tgt_keypts
    ([B,N,3] tensors, or lists of per-pair [N,3] tensors) -> {"final_trans": [B,4,4], "final_labels": per-pair [N] rows}.  A ragged
    group is ONE batched device call (``ransac.ransac_correspondence``), not a loop.  ``data["pair_offset"]`` (optional; eval_scene
    passes the index of the group's first pair) keeps a pair's draws independent of the grouping."""
    wants_pair_offset = True

    def __init__(self, inlier_threshold: float = 0.10, ransac_n: int = 4, max_iteration: int = 1000, seed: int = 0):
        self.inlier_threshold, self.ransac_n = float(inlier_threshold), int(ransac_n)
        self.max_iteration, self.seed = int(max_iteration), int(seed)

    def __call__(self, data):
        trans, labels = ransac_correspondence(data["src_keypts"], data["tgt_keypts"], self.inlier_threshold, ransac_n=self.ransac_n,
                                              max_iteration=self.max_iteration, seed=self.seed,
                                              pair_offset=int(data.get("pair_offset", 0)))
        return {"final_trans": trans, "final_labels": labels}


SOLVERS = ("SVD", "RANSAC")


def eval_scene(model, pairs: Iterable[Dict[str, np.ndarray]], scene_ind: int = 0, re_thre: float = 15.0, te_thre: float = 30.0,
               inlier_threshold: float = 0.10, use_mutual: bool = False, device: str = "cuda:0", batch_size: int = 1,
               use_icp: bool = False, icp_distance: float = 0.10, corr_batch: bool = False, solver: str = "SVD") -> np.ndarray:
    """`pairs`: dicts with src_pts [ns,3], tgt_pts [nt,3], src_desc [ns,D], tgt_desc [nt,D], gt_trans [4,4] (numpy).
    Returns the [num_pair, 12] stats array of the reference's eval_3DMatch_scene.
    batch_size > 1 (r03): the correspondence sets of `batch_size` consecutive pairs -- every pair has its own N, as in the
    reference's evaluation (test_3DMatch.py:126 `num_node='all'`) -- go through ONE ragged call of the model (lists of
    per-pair tensors); model / data time are then the batch's time divided by its pairs.
    use_icp (test_3DMatch.py:79-80): the predicted poses are refined by point-to-point ICP of the correspondence endpoints
    (benchmark_utils.icp_refine, max_correspondence_distance = icp_distance) -- the group's pairs in one ragged device call,
    inside the model time as in the reference; the stats rows then use the refined poses.
    corr_batch (f-19; with batch_size > 1): the group's correspondences and ground-truth labels come from one
    `build_correspondences_batch` call (labels in fp64, datasets/ThreeDMatch.py:293-297, where the per-pair path uses
    `gt_labels_from_trans`' fp32); data time is then the group's time divided by its pairs.
    solver (test_3DMatch.py:59-77 `--solver`): "SVD" keeps the model's pose; "RANSAC" replaces the group's poses and labels by
    `ransac_correspondence` (ransac_n 3, 5000 iterations) over the correspondences the model labelled as inliers -- one ragged device
    call after the forward and before use_icp, inside the model time, with no host read.  Its draws are numbered by the pair's index
    in the scene, so batch_size does not change a pair's result."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    rows: List[np.ndarray] = []
    dev = torch.device(device)
    g = lambda a: a.to(dev) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def flush(group):
        if not group:
            return
        t0 = time.perf_counter()
        first = len(rows)                                                  # index of the group's first pair in the scene
        extra = {"pair_offset": first} if getattr(model, "wants_pair_offset", False) else {}
        if len(group) == 1:
            c = group[0]["corr"]
            res = model({"corr_pos": c["corr_pos"], "src_keypts": c["src_keypts"], "tgt_keypts": c["tgt_keypts"], "testing": True,
                         **extra})                                                                         # test_3DMatch.py:53
            trans, labels = res["final_trans"], [res["final_labels"][0]]
        else:
            res = model({"corr_pos": [x["corr"]["corr_pos"][0] for x in group], "src_keypts": [x["corr"]["src_keypts"][0] for x in group],
                         "tgt_keypts": [x["corr"]["tgt_keypts"][0] for x in group], "testing": True, **extra})
            trans, labels = res["final_trans"], res["final_labels"]
        if solver == "RANSAC":                                                                             # test_3DMatch.py:59-77
            trans, labels = ransac_correspondence([x["corr"]["src_keypts"][0] for x in group], [x["corr"]["tgt_keypts"][0] for x in group],
                                                  inlier_threshold, ransac_n=3, max_iteration=5000, mask=list(labels),
                                                  pair_offset=first)
        if use_icp:                                                                                        # test_3DMatch.py:79-80
            trans = icp_refine([x["corr"]["src_keypts"][0] for x in group], [x["corr"]["tgt_keypts"][0] for x in group], trans,
                               icp_distance)
        torch.cuda.synchronize(dev)
        model_time = (time.perf_counter() - t0) / len(group)
        for i, x in enumerate(group):
            st = ops.eval_stats(trans[i:i + 1], x["gt_trans"][None], labels[i][None], x["gt_labels"], re_thre, te_thre)[0].cpu().numpy()
            row = np.zeros(12)
            row[:9] = st
            row[9], row[10], row[11] = model_time, x["data_time"], scene_ind
            rows.append(row)

    def build_group(raw):
        """corr_batch: the correspondences and labels of the group's pairs from ONE batched call (pool = the pairs' clouds in turn)."""
        t0 = time.perf_counter()
        desc = [g(x[k]) for x in raw for k in ("src_desc", "tgt_desc")]
        pts = [g(x[k]) for x in raw for k in ("src_pts", "tgt_pts")]
        gt64 = torch.stack([torch.as_tensor(np.asarray(x["gt_trans"].cpu() if torch.is_tensor(x["gt_trans"]) else x["gt_trans"],
                                                       dtype=np.float64)) for x in raw])
        c = build_correspondences_batch(desc, pts, [(2 * i, 2 * i + 1) for i in range(len(raw))], use_mutual=use_mutual,
                                        gt_trans=gt64, inlier_threshold=inlier_threshold)
        counts = c["num_corr"].tolist() if use_mutual else c["num_corr_host"]
        torch.cuda.synchronize(dev)
        data_time = (time.perf_counter() - t0) / len(raw)
        return [{"corr": {k: c[k][i:i + 1, :n] for k in ("corr_pos", "src_keypts", "tgt_keypts")}, "gt_trans": g(x["gt_trans"]).float(),
                 "gt_labels": c["gt_labels"][i:i + 1, :n], "data_time": data_time} for i, (x, n) in enumerate(zip(raw, counts))]

    with torch.no_grad():
        group = []
        if corr_batch and batch_size > 1:
            for pair in pairs:
                group.append(pair)
                if len(group) >= batch_size:
                    flush(build_group(group))
                    group = []
            if group:
                flush(build_group(group))
            return np.stack(rows) if rows else np.zeros((0, 12))
        for pair in pairs:
            t0 = time.perf_counter()
            corr = build_correspondences(g(pair["src_desc"]), g(pair["tgt_desc"]), g(pair["src_pts"]), g(pair["tgt_pts"]),
                                         use_mutual=use_mutual)
            gt_trans = g(pair["gt_trans"]).float()
            gt_labels = gt_labels_from_trans(corr["src_keypts"][0], corr["tgt_keypts"][0], gt_trans, inlier_threshold)[None]
            torch.cuda.synchronize(dev)
            group.append({"corr": corr, "gt_trans": gt_trans, "gt_labels": gt_labels, "data_time": time.perf_counter() - t0})
            if len(group) >= max(1, batch_size):
                flush(group)
                group = []
        flush(group)
    return np.stack(rows) if rows else np.zeros((0, 12))


def summarize(stats: np.ndarray) -> Dict[str, float]:
    """The aggregate lines of eval_3DMatch (evaluation/test_3DMatch.py:141-176)."""
    ok = stats[:, 0] > 0
    return {
        "num_pairs": int(len(stats)),
        "registration_recall_pct": float(stats[:, 0].mean() * 100.0) if len(stats) else float("nan"),
        "mean_RE_deg_success": float(stats[ok, 1].mean()) if ok.any() else float("nan"),
        "mean_TE_cm_success": float(stats[ok, 2].mean()) if ok.any() else float("nan"),
        "mean_input_inlier_ratio_pct": float(stats[:, 4].mean() * 100.0) if len(stats) else float("nan"),
        "mean_precision_pct": float(stats[:, 6].mean() * 100.0) if len(stats) else float("nan"),
        "mean_recall_pct": float(stats[:, 7].mean() * 100.0) if len(stats) else float("nan"),
        "mean_f1_pct": float(stats[:, 8].mean() * 100.0) if len(stats) else float("nan"),
        "mean_model_time_s": float(stats[:, 9].mean()) if len(stats) else float("nan"),
        "mean_data_time_s": float(stats[:, 10].mean()) if len(stats) else float("nan"),
    }


def _check_descriptor(descriptor: str) -> bool:
    if descriptor not in ("standin", "fpfh"):
        raise ValueError(f"descriptor must be 'standin' or 'fpfh', got {descriptor!r}")
    return descriptor == "fpfh"


def device_fpfh(points: np.ndarray, voxel: float, device: str = "cuda:0") -> torch.Tensor:
    """FPFH descriptors [n,33] fp32 of a cloud down-sampled at `voxel`, computed and left on the device (f-7)."""
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(torch.device(device))
    return fpfh_descriptors(pts[None], voxel)[0]


def device_demo_fpfh(raw_points: np.ndarray, voxel: float, device: str = "cuda:0") -> Tuple[torch.Tensor, torch.Tensor]:
    """The demo's ``extract_fpfh_features`` (demo_registration.py:37-44) on a RAW cloud (f-9): the vertices go to the device as they
    are, normals are estimated on them, the cloud is down-sampled at `voxel` with averaged normals, and FPFH is computed on the
    result.  Nothing is down-sampled on the host.  Returns (points [n,3] fp32, desc [n,33] fp32), both left on the device."""
    pts = torch.from_numpy(np.ascontiguousarray(raw_points, dtype=np.float32)).to(torch.device(device))
    res = extract_fpfh_features(pts[None], voxel)
    n = max(0, int(res["counts"][0].item()))
    return res["points"][0, :n], res["desc"][0, :n]


def demo_pairs(cloud: np.ndarray, num_pairs: int, dim: int = 33, cell: float = 0.05, corrupt: float = 0.6,
               seed: int = 0, descriptor: str = "standin", voxel: float = 0.05, device: str = "cuda:0") -> Iterable[Dict[str, np.ndarray]]:
    """Pairs for the loop from ONE down-sampled cloud: view i = `second_view(cloud, seed + i)`; stand-in descriptors, or with
    descriptor="fpfh" the device's FPFH of each view (cloud down-sampled at `voxel`; descriptors stay on `device`)."""
    fpfh = _check_descriptor(descriptor)
    src_desc = device_fpfh(cloud, voxel, device) if fpfh else None
    for i in range(num_pairs):
        rs = np.random.RandomState(10_000 + seed + i)
        tgt, T, tgt_in_src = second_view(cloud, seed + i)
        if fpfh:
            yield {"src_pts": cloud, "tgt_pts": tgt, "gt_trans": T, "src_desc": src_desc, "tgt_desc": device_fpfh(tgt, voxel, device)}
            continue
        yield {"src_pts": cloud, "tgt_pts": tgt, "gt_trans": T,
               "src_desc": standin_descriptors(cloud, dim, cell, seed + i, corrupt, rs),
               "tgt_desc": standin_descriptors(tgt_in_src, dim, cell, seed + i, corrupt * 0.5, rs)}


# ---------------------------------------------------------------------------------------------------------------
# the multiway driver's pair loop (multiway/test_multi_ate.py:98-157)
# ---------------------------------------------------------------------------------------------------------------
def demo_views(cloud: np.ndarray, num_views: int, dim: int = 33, cell: float = 0.05, corrupt: float = 0.4, seed: int = 0,
               odometry_deg: float = 2.0, odometry_cm: float = 5.0, descriptor: str = "standin", voxel: float = 0.05,
               device: str = "cuda:0") -> List[Dict[str, np.ndarray]]:
    """Fragments for `multiway_edges` from ONE down-sampled cloud, built like `demo_pairs`: view i = `second_view(cloud, seed + i)`
    in its own frame, with stand-in descriptors that agree between the views for points of the same cell of the cloud's frame
    (descriptor="fpfh": the device's FPFH of each view, as in `demo_pairs`).
    `pose` [4,4]: p_view = pose p_cloud.  `odometry` [4,4] (all but the last view): the motion onto the next view disturbed by
    `odometry_deg` / `odometry_cm` -- the stand-in for the fragment odometry the driver starts its local refinement from
    (multiway/test_multi_ate.py:119-121)."""
    fpfh = _check_descriptor(descriptor)
    views = []
    for i in range(num_views):
        rs = np.random.RandomState(20_000 + seed + i)
        pts, T, in_cloud = second_view(cloud, seed + i)
        desc = device_fpfh(pts, voxel, device) if fpfh else standin_descriptors(in_cloud, dim, cell, seed, corrupt, rs)
        views.append({"pts": pts, "pose": T.astype(np.float64), "desc": desc})
    for i in range(num_views - 1):
        rs = np.random.RandomState(30_000 + seed + i)
        axis = rs.standard_normal(3)
        axis /= np.linalg.norm(axis)
        a = np.radians(odometry_deg)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        D = np.eye(4)
        D[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        d = rs.standard_normal(3)
        D[:3, 3] = d / np.linalg.norm(d) * odometry_cm / 100.0
        views[i]["odometry"] = (D @ views[i + 1]["pose"] @ np.linalg.inv(views[i]["pose"])).astype(np.float32)
    return views


def multiway_edges(model, views: List[Dict[str, np.ndarray]], use_mutual: bool = False, device: str = "cuda:0", batch_pairs: int = 1):
    """The pairwise-registration loop of the multiway driver (multiway/test_multi_ate.py:98-157) over `views` (dicts with pts [n,3],
    desc [n,D] and, for every view but the last, odometry [4,4]; `demo_views` builds them): every pair s < t in the driver's order.
      t == s + 1 (odometry case, :117-135): `local_refinement` of the full clouds from views[s]['odometry'] -> a certain edge;
      otherwise (:136-154): match -> `model(data)` -> `loop_closure_edge`; a pair the gate drops is skipped, the others are
      uncertain edges.
    Everything up to the gate stays on the device; the gates of all pairs are read back once, at the end.
    batch_pairs > 1: the loop closures run `batch_pairs` at a time through the batched correspondence construction and one ragged
    forward per group (`_pairwise_registration`); the same edges in the same order.
    Returns the edges as the driver would append them: tuples (s, t, T [4,4] float64 numpy, info [6,6] float64 numpy, uncertain)."""
    dev = torch.device(device)
    found, _ = _pairwise_registration(model, views, use_mutual, dev, batch_pairs)
    keep = torch.stack([f[4] if f[4] is not None else torch.ones((), dtype=torch.bool, device=dev) for f in found]).cpu().numpy()
    return [(s, t, T.double().cpu().numpy(), info.cpu().numpy(), gate is not None)
            for (s, t, T, info, gate), k in zip(found, keep) if k]


def _pairwise_registration(model, views, use_mutual: bool, dev, batch_pairs: int = 1):
    """The pair loop of `multiway_edges`, everything left on the device: -> ([(s, t, T [4,4] fp32, info [6,6] fp64, gate or None)] in
    the driver's order -- gate: the overlap gate's 0-d bool tensor of a loop closure, None for an odometry edge --, the views' points).
    batch_pairs > 1 (f-19): the loop-closure candidates are taken `batch_pairs` at a time, in the driver's order: one
    `build_correspondences_batch` over the views' pool, one forward with `num_corr`, one `loop_closure_edge` per group.  The
    group's counts are known from the shapes; with the mutual check they are read once per group."""
    g = lambda a: a.to(dev).float() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    pts = [g(v["pts"]) for v in views]
    desc = [g(v["desc"]) for v in views]
    found = []
    pool = CorrPool(desc, pts) if batch_pairs > 1 else None
    group = []                                       # (position in found, s, t) of the candidates waiting for their group

    def flush():
        if not group:
            return
        c = build_correspondences_batch(pool, None, [(s, t) for _, s, t in group], use_mutual=use_mutual)
        counts = c["num_corr"].tolist() if use_mutual else c["num_corr_host"]
        res = model({"corr_pos": c["corr_pos"], "src_keypts": c["src_keypts"], "tgt_keypts": c["tgt_keypts"], "num_corr": counts,
                     "testing": True})
        edge = loop_closure_edge([c["src_keypts"][i, :n] for i, n in enumerate(counts)],
                                 [c["tgt_keypts"][i, :n] for i, n in enumerate(counts)], res["final_trans"])
        for i, (pos, s, t) in enumerate(group):
            found[pos] = (s, t, res["final_trans"][i], edge["information"][i], edge["keep"][i])
        group.clear()

    with torch.no_grad():
        for s in range(len(views)):
            for t in range(s + 1, len(views)):
                if t == s + 1:
                    T, info = local_refinement(pts[s][None], pts[t][None], g(views[s]["odometry"])[None])
                    found.append((s, t, T[0], info[0], None))
                elif batch_pairs > 1:
                    group.append((len(found), s, t))
                    found.append(None)
                    if len(group) >= batch_pairs:
                        flush()
                else:
                    c = build_correspondences(desc[s], desc[t], pts[s], pts[t], use_mutual=use_mutual)
                    res = model({"corr_pos": c["corr_pos"], "src_keypts": c["src_keypts"], "tgt_keypts": c["tgt_keypts"], "testing": True})
                    edge = loop_closure_edge(c["src_keypts"], c["tgt_keypts"], res["final_trans"])
                    found.append((s, t, res["final_trans"][0], edge["information"][0], edge["keep"][0]))
        flush()
    return found, pts


def multiway_trajectory(model, views: List[Dict[str, np.ndarray]], use_icp: bool = False, use_mutual: bool = False,
                        device: str = "cuda:0", return_graph: bool = False, batch_pairs: int = 1) -> Dict[str, object]:
    """The driver's `eval_redwood_scene` plus its ATE (multiway/test_multi_ate.py:86-227, :262-270) over `views` (as `multiway_edges`
    takes them; `pose` [4,4] is the ground truth: p_view = pose p_scene):
      1. the edges of `multiway_edges` (`batch_pairs` as there), with the overlap gates kept on the device and handed to the optimiser
         as its edge mask;
      2. the node chain over the odometry edges (:129-130);
      3. `global_optimization` (:166-174);
      4. use_icp (:188-224): `multi_scale_icp` of every edge from its transformation on the full clouds (the pruned ones too: which
         edges survived is known on the device only; they stay masked out), the node chain again, a second `global_optimization`;
      5. `align` of the node origins onto the views' true origins and sqrt(mean(err^2)).
    Nothing is read on the host before the final ATE.  Returns ate_cm, errors_cm [F] (device), nodes_before / nodes_after,
    edges_before / edges_after (as the driver prints them), nodes [F,4,4], keep [E], confidence [E], record [12] (device tensors; with
    use_icp those of the second optimisation, plus first_record); return_graph adds graph = the inputs of the last optimisation
    (nodes, edges, edge_mask)."""
    from .multiway import align, global_optimization, multi_scale_icp, pose_graph_nodes
    dev = torch.device(device)
    F = len(views)
    found, pts = _pairwise_registration(model, views, use_mutual, dev, batch_pairs)
    with torch.no_grad():
        edges = {"source": torch.tensor([f[0] for f in found], dtype=torch.int32).to(dev),
                 "target": torch.tensor([f[1] for f in found], dtype=torch.int32).to(dev),
                 "transformation": torch.stack([f[2] for f in found]), "information": torch.stack([f[3] for f in found]),
                 "uncertain": torch.tensor([f[4] is not None for f in found]).to(dev)}
        mask = torch.stack([f[4] if f[4] is not None else torch.ones((), dtype=torch.bool, device=dev) for f in found])
        nodes = pose_graph_nodes(edges, F, edge_mask=mask)
        res = global_optimization(nodes, edges, edge_mask=mask)
        out = {}
        if use_icp:
            out["first_record"] = res["record"]
            refined = [multi_scale_icp(pts[s][None], pts[t][None], trans=T[None]) for s, t, T, _, _ in found]
            edges = dict(edges, transformation=torch.cat([r["transformation_f64"] for r in refined]),
                         information=torch.cat([r["information"] for r in refined]))
            mask = res["keep"]
            nodes = pose_graph_nodes(edges, F, edge_mask=mask)
            res = global_optimization(nodes, edges, edge_mask=mask)
        truth = np.stack([np.linalg.inv(np.asarray(v["pose"], dtype=np.float64))[:3, 3] for v in views], axis=1)
        _, err = align(res["nodes"][:, :3, 3].T.contiguous(), torch.from_numpy(truth).to(dev))
        ate = torch.sqrt((err.double() ** 2).mean())
        record = res["record"].cpu().numpy()                   # the one read-back: record and ATE
    out.update(ate_cm=float(ate), errors_cm=err, nodes_before=F, nodes_after=F, edges_before=int(record[9]), edges_after=int(record[11]),
               nodes=res["nodes"], keep=res["keep"], confidence=res["confidence"], record=res["record"])
    if return_graph:
        out["graph"] = {"nodes": nodes, "edges": edges, "edge_mask": mask}
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the validation loop (libs/trainer.py:158-222)
# ---------------------------------------------------------------------------------------------------------------------------
VALIDATE_NAMES = ("class_loss", "trans_loss", "sm_loss", "reg_recall", "re", "te", "precision", "recall", "f1")


def validate(model, batches: Iterable[Dict[str, torch.Tensor]], balanced: bool = False, re_thre: float = 15.0,
             te_thre: float = 30.0) -> Dict[str, float]:
    """``Trainer.evaluate`` (libs/trainer.py:158-222) on the device: for every batch (dict with corr_pos [bs,N,in_dim], src_keypts,
    tgt_keypts [bs,N,3], gt_trans [bs,4,4], gt_labels [bs,N]) the validation forward of `model` (eval() mode) and the three losses
    of pointdsc_amd.losses on its outputs.  The nine meters of the reference are running means kept on the device (fp64; a NaN
    value is skipped, as the reference's `if not np.isnan(...)` does); ONE device -> host copy at the end returns them all.
    The spectral-matching loss is also taken straight from the forward's normalised features (workspace entry "normed") without
    reading M; that value is returned as "sm_loss_features" and equals "sm_loss" bit for bit.
    The reference logs ``te`` as ``float(re)`` (libs/trainer.py:203); the REAL translation error is returned here."""
    from .losses import classification_loss_raw, sm_loss_features_raw, sm_loss_matrix_raw, transformation_loss_raw
    dev = next(model.parameters()).device
    names = VALIDATE_NAMES + ("sm_loss_features",)
    sums = torch.zeros(len(names), device=dev, dtype=torch.float64)
    counts = torch.zeros(len(names), device=dev, dtype=torch.float64)
    with torch.no_grad():
        for batch in batches:
            d = {k: v.to(dev) for k, v in batch.items() if torch.is_tensor(v)}
            res = model({k: d[k] for k in ("corr_pos", "src_keypts", "tgt_keypts")})
            logits, gt = res["final_labels"], d["gt_labels"]
            bs, n = logits.shape
            cls = classification_loss_raw(logits, gt, None, balanced)[0]
            sm = sm_loss_matrix_raw(res["M"], gt, balanced)[0]
            normed = model.workspace_view("normed", bs, n)[: bs * n * 128].view(bs * n, 128)
            smf = sm_loss_features_raw(normed, model.sigma, gt, balanced)[0]
            tr = transformation_loss_raw(res["final_trans"], d["gt_trans"], d["src_keypts"], d["tgt_keypts"], logits, re_thre, te_thre)
            vals = torch.stack([cls[0], tr[0], sm[0], tr[1], tr[2], tr[3], cls[1], cls[2], cls[3], smf[0]])
            ok = ~torch.isnan(vals)
            sums += torch.where(ok, vals, torch.zeros_like(vals))
            counts += ok.to(torch.float64)
        means = (sums / counts).cpu().tolist()          # the one read-back (a meter that never got a value is NaN)
    return dict(zip(names, means))


# ---------------------------------------------------------------------------------------------------------------------------
# the training loop (libs/trainer.py:79-136)
# ---------------------------------------------------------------------------------------------------------------------------
def train_epoch(model, batches: Iterable[Dict[str, torch.Tensor]], optimizer, weights=(1.0, 1.0, 0.0), balanced: bool = False,
                re_thre: float = 15.0, te_thre: float = 30.0) -> Dict[str, float]:
    """``Trainer.train_epoch`` (libs/trainer.py:79-136) on the device: for every batch (the dict ``validate`` takes) zero_grad, the
    train()-mode forward of `model` (a ``training.TrainablePointDSC`` in train() mode), the three losses of pointdsc_amd.losses,
    ``weights[0] class_loss + weights[1] sm_loss``, backward, and the reference's rule that the optimiser step is skipped when any
    gradient is non-finite (one boolean per step is read for it, as the reference reads one; with a ``pointdsc_amd.DeviceAdam`` /
    ``DeviceSGD`` whose guard is on, the optimiser makes that decision on the device and the loop reads nothing back).  `balanced` is the reference's
    config.balanced (default False).  ``weights[2]`` is the reference's weight_transformation (libs/trainer.py:105-107; default 0.0,
    and the caller keeps it 0 until transformation_loss_start_epoch): above 0 the model must have been built with
    ``differentiable_trans=True``, so that its final_trans carries a gradient, and ``weights[2] * trans_loss`` joins the objective;
    for any other model a weight above 0 raises NotImplementedError.  With weight 0 the transformation loss is a meter only.
    -> the nine meters of the reference (running means kept on the device in fp64, NaN values skipped, as in ``validate``), and
    "loss_first" / "loss_last" (the weighted sum at the first and the last step), "steps", "skipped" -- ONE read-back at the end."""
    from .losses import ClassificationLoss, SpectralMatchingLoss, TransformationLoss, transformation_loss_raw
    from .optim import DeviceAdam, DeviceSGD
    w_cls, w_sm, w_tr = (float(w) for w in weights)
    if w_tr > 0.0 and not getattr(model, "differentiable_trans", False):
        raise NotImplementedError("a transformation-loss weight above 0 needs a final_trans with a gradient: build the model as "
                                  "TrainablePointDSC(..., differentiable_trans=True), or use weight 0.0, the reference's default")
    if not model.training:
        raise RuntimeError("train_epoch needs the model in train() mode")
    dev = next(model.parameters()).device
    cls_fn, sm_fn, tr_fn = ClassificationLoss(balanced), SpectralMatchingLoss(balanced), TransformationLoss(re_thre, te_thre)
    params = [p for p in model.parameters() if p.requires_grad]
    sums = torch.zeros(len(VALIDATE_NAMES), device=dev, dtype=torch.float64)
    counts = torch.zeros(len(VALIDATE_NAMES), device=dev, dtype=torch.float64)
    totals, steps, skipped = [], 0, 0
    # a DeviceAdam / DeviceSGD with its guard on decides the skip on the device: no boolean is read inside the loop, and the number
    # of skipped steps (its device counter, now minus at entry) joins the one read-back at the end
    on_device = isinstance(optimizer, (DeviceAdam, DeviceSGD)) and optimizer.guard
    skipped_at_entry = optimizer.skipped_steps() if on_device else None
    for batch in batches:
        d = {k: v.to(dev) for k, v in batch.items() if torch.is_tensor(v)}
        gt = d["gt_labels"]
        optimizer.zero_grad()
        res = model({k: d[k] for k in ("corr_pos", "src_keypts", "tgt_keypts")})
        logits = res["final_labels"]
        cls = cls_fn(logits, gt, device_stats=True)
        sm = sm_fn(res["M"], gt)
        loss = w_cls * cls["loss"] + w_sm * sm
        tr = None
        if w_tr > 0.0:
            tr = tr_fn(res["final_trans"], d["gt_trans"], d["src_keypts"], d["tgt_keypts"], logits, device_stats=True)
            loss = loss + w_tr * tr[0]
        loss.backward()
        if on_device:
            optimizer.step()
        else:
            grads = [p.grad for p in params if p.grad is not None]
            if bool(torch.stack([torch.isfinite(g).all() for g in grads]).all()):
                optimizer.step()
            else:
                skipped += 1
        steps += 1
        with torch.no_grad():
            if tr is None:
                tr = transformation_loss_raw(res["final_trans"], d["gt_trans"], d["src_keypts"], d["tgt_keypts"], logits, re_thre, te_thre)
            vals = torch.stack([cls["loss"].detach().double(), tr[0].detach().double(), sm.detach().double(), tr[1], tr[2], tr[3],
                                cls["precision"], cls["recall"], cls["f1"]])
            ok = ~torch.isnan(vals) & ~torch.isnan(loss.detach())          # the reference updates no meter on a NaN loss
            sums += torch.where(ok, vals, torch.zeros_like(vals))
            counts += ok.to(torch.float64)
            totals.append(loss.detach().double())
    if not steps:
        raise ValueError("train_epoch: no batch")
    tail = [totals[0], totals[-1]]
    if on_device:
        tail.append((optimizer.skipped_steps() - skipped_at_entry).double())
    out = torch.cat([sums / counts, torch.stack(tail)]).cpu().tolist()          # the one read-back
    if on_device:
        skipped = int(out.pop())
    res = dict(zip(VALIDATE_NAMES, out))
    res.update(loss_first=out[-2], loss_last=out[-1], steps=steps, skipped=skipped)
    return res
