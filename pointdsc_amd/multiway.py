"""The multiway driver's edge step on the device: what ``multiway/test_multi_ate.py`` does around
``model(data)`` with open3d on the host -- the edge's information matrix and overlap gate (:141-149), multi-scale ICP of
the odometry edges (:54-83) and the trajectory alignment of its ATE (:31-51).  Pose-graph optimisation
(``o3d.registration.global_optimization``, a host-side LM solver over the edges) is not part of it.

The arithmetic runs in libpointdsc_hip.so (``pdsc_information_matrix``, ``pdsc_voxel_keys`` / ``pdsc_voxel_means``,
``pdsc_icp_refine``); nothing here reads a device value on the host, so per-pair point counts stay on the device from one
scale to the next.  GPU only.

Point clouds are ``[bs,N,3]`` tensors or lists of per-pair ``[n_b,3]`` tensors, as in ``pointdsc_amd.icp``.

Documented difference: open3d keeps the fp64 voxel means for its ICP; ``registration_icp`` takes fp32 points, so the means
are rounded to fp32 once (at most 6e-8 relative).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .icp import Points, _as_batch, _as_poses, _counts, _pair_batches, registration_icp
from .ops import _on_device, _p, _stream

# multiway/test_multi_ate.py:60, :144 and :167 (0.05 is the 3DMatch voxel size)
EDGE_DISTANCE = 0.05 * 1.4
MIN_OVERLAP = 0.30                                  # :147
VOXEL_SIZES = (0.05, 0.05 / 2.0, 0.05 / 4.0)        # :80
MAX_ITERS = (50, 30, 14)                            # :81


@_on_device
def information_matrix(source: Points, target: Points, max_correspondence_distance: float, transformation: torch.Tensor,
                       source_counts: Optional[torch.Tensor] = None, target_counts: Optional[torch.Tensor] = None,
                       return_correspondences: bool = False) -> Dict[str, torch.Tensor]:
    """open3d ``registration.get_information_matrix_from_point_clouds(source, target, max_correspondence_distance,
    transformation)`` for every pair of the batch; ``transformation`` [bs,4,4] or [4,4] fp32.

    Returns ``information`` [bs,6,6] fp64 (the plain sum: IDENTITY_RULE of the header) and ``num_correspondences`` [bs] int32;
    with ``return_correspondences`` also ``correspondences`` [bs,Ns] int32 (target index per source point, -1 = none)."""
    lib = _lib.load()
    if math.isnan(float(max_correspondence_distance)):
        raise ValueError("max_correspondence_distance is NaN")
    src, tgt, ns_dev, nt_dev = _pair_batches(source, target, source_counts, target_counts)
    bs, dev = src.shape[0], src.device
    trans = _as_poses(transformation, bs, "transformation")
    Ns, Nt = int(src.shape[1]), int(tgt.shape[1])
    ws_bytes = int(lib.pdsc_information_workspace_bytes(bs, Ns, Nt))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    info = torch.empty(bs, 6, 6, dtype=torch.float64, device=dev)
    ncorr = torch.empty(bs, dtype=torch.int32, device=dev)
    corr = torch.empty(bs, Ns, dtype=torch.int32, device=dev) if return_correspondences else None
    _lib.check(lib.pdsc_information_matrix(_p(src), _p(tgt), _p(trans), _p(ns_dev), _p(nt_dev), float(max_correspondence_distance),
                                           _p(info), _p(ncorr), _p(corr), _p(ws), ws_bytes, bs, Ns, Nt, _stream()),
               "pdsc_information_matrix")
    out = {"information": info, "num_correspondences": ncorr}
    if return_correspondences:
        out["correspondences"] = corr
    return out


@_on_device
def voxel_down_sample(points: Points, voxel_size: float, counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """open3d ``PointCloud.voxel_down_sample(voxel_size)`` of every cloud of the batch, as ``harness.voxel_down_sample`` restates
    it (one point per occupied voxel = the fp64 mean rounded to fp32, ordered by voxel index).

    Returns ``(padded [bs,n,3] fp32, counts [bs] int32 on the device)``: ``n`` is the input's row count, rows beyond a cloud's
    count are zero.  The counts are not read on the host.  A cloud with a non-finite point comes back with count 0."""
    lib = _lib.load()
    v = float(voxel_size)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    pts, _, n_dev = _as_batch(points, "points")
    bs, n = int(pts.shape[0]), int(pts.shape[1])
    if counts is not None:
        if n_dev is not None:
            raise ValueError("counts goes with a padded [bs,N,3] tensor, not with a list of clouds")
        n_dev = _counts(counts, bs, pts.device, "counts")
    keys = torch.empty(bs, n, dtype=torch.int64, device=pts.device)
    _lib.check(lib.pdsc_voxel_keys(_p(pts), _p(n_dev), v, _p(keys), bs, n, _stream()), "pdsc_voxel_keys")
    sorted_keys, perm = torch.sort(keys, dim=1, stable=True)        # plumbing; keys and means are the library's
    out = torch.empty(bs, n, 3, dtype=torch.float32, device=pts.device)
    out_counts = torch.empty(bs, dtype=torch.int32, device=pts.device)
    _lib.check(lib.pdsc_voxel_means(_p(pts), _p(sorted_keys.contiguous()), _p(perm.contiguous()), _p(out), _p(out_counts), bs, n,
                                    _stream()), "pdsc_voxel_means")
    return out, out_counts


def _trace_f32(T: torch.Tensor) -> torch.Tensor:
    """numpy's ``trace()`` of an fp32 4x4: the sequential fp32 sum of the diagonal."""
    return ((T[:, 0, 0] + T[:, 1, 1]) + T[:, 2, 2]) + T[:, 3, 3]


def overlap_gate(information: torch.Tensor, transformation: torch.Tensor, min_points: torch.Tensor,
                 min_overlap: float = MIN_OVERLAP) -> torch.Tensor:
    """multiway/test_multi_ate.py:147, negated: keep = not (information[5,5] / min(Ns, Nt) < min_overlap or trace(T) == 4.0).
    ``min_points`` [bs]: min(Ns_b, Nt_b).  Works on any device (element-wise torch)."""
    ratio = information[:, 5, 5] / min_points.to(torch.float64)
    return ~((ratio < min_overlap) | (_trace_f32(transformation) == 4.0))


@_on_device
def loop_closure_edge(src_keypts: Points, tgt_keypts: Points, pred_trans: torch.Tensor,
                      max_correspondence_distance: float = EDGE_DISTANCE, min_overlap: float = MIN_OVERLAP) -> Dict[str, torch.Tensor]:
    """multiway/test_multi_ate.py:141-149 for a batch of loop-closure candidates: the information matrix of the forward's pose
    over the correspondence endpoints, and ``keep`` [bs] bool on the device (False = "too small overlapping", the driver's
    ``continue``)."""
    res = information_matrix(src_keypts, tgt_keypts, max_correspondence_distance, pred_trans)
    ns = _point_counts(src_keypts, res["information"].device)
    nt = _point_counts(tgt_keypts, res["information"].device)
    trans = _as_poses(pred_trans, int(ns.shape[0]), "pred_trans")
    res["keep"] = overlap_gate(res["information"], trans, torch.minimum(ns, nt), min_overlap)
    return res


def _point_counts(x: Points, dev) -> torch.Tensor:
    if torch.is_tensor(x):
        return torch.full((int(x.shape[0]),), int(x.shape[1]), dtype=torch.int32, device=dev)
    return torch.tensor([int(t.shape[-2]) for t in x], dtype=torch.int32).to(dev, non_blocking=True)


@_on_device
def multi_scale_icp(src: Points, tgt: Points, voxel_size: Sequence[float] = VOXEL_SIZES, max_iter: Sequence[int] = MAX_ITERS,
                    trans: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """multiway/test_multi_ate.py:54-73 for a batch of pairs: per scale, down-sample both clouds on the device and run
    point-to-point ICP (distance 0.05 * 1.4, ``max_iteration = max_iter[scale]``, default relative criteria) from the previous
    scale's pose rounded to fp32; after the last scale, the information matrix at ``voxel_size[-1] * 1.4``.

    Returns ``transformation`` [bs,4,4] fp32, ``transformation_f64``, ``information`` [bs,6,6] fp64, ``num_correspondences``
    and ``scales``: per scale the ``registration_icp`` record plus ``source_down`` / ``target_down`` / ``source_counts`` /
    ``target_counts``.  No host synchronisation between the scales."""
    if len(voxel_size) < len(max_iter) or len(max_iter) < 1:
        raise ValueError(f"{len(max_iter)} scales need as many voxel sizes, got {len(voxel_size)}")
    for v in voxel_size[:len(max_iter)]:
        if not (float(v) > 0.0 and math.isfinite(float(v))):
            raise ValueError(f"voxel_size must be positive and finite, got {v}")
    s_pts, t_pts, ns_dev, nt_dev = _pair_batches(src, tgt)
    bs = int(s_pts.shape[0])
    if trans is None:
        trans = torch.eye(4, dtype=torch.float32, device=s_pts.device)
    current = _as_poses(trans, bs, "trans")
    scales: List[Dict[str, object]] = []
    for scale in range(len(max_iter)):
        s_down, s_n = voxel_down_sample(s_pts, voxel_size[scale], ns_dev)
        t_down, t_n = voxel_down_sample(t_pts, voxel_size[scale], nt_dev)
        res = registration_icp(s_down, t_down, current, EDGE_DISTANCE, max_iteration=int(max_iter[scale]),
                               source_counts=s_n, target_counts=t_n)
        res.update(source_down=s_down, target_down=t_down, source_counts=s_n, target_counts=t_n, voxel_size=float(voxel_size[scale]))
        scales.append(res)
        current = res["transformation"]
    last = scales[-1]
    info = information_matrix(last["source_down"], last["target_down"], last["voxel_size"] * 1.4, current,
                              last["source_counts"], last["target_counts"])
    return {"transformation": current, "transformation_f64": last["transformation_f64"], "information": info["information"],
            "num_correspondences": info["num_correspondences"], "scales": scales}


def local_refinement(src: Points, tgt: Points, trans: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """multiway/test_multi_ate.py:76-83: ``multi_scale_icp`` at voxel sizes 0.05 / 0.025 / 0.0125 with 50 / 30 / 14 iterations
    -> (transformation [bs,4,4] fp32, information [bs,6,6] fp64)."""
    res = multi_scale_icp(src, tgt, VOXEL_SIZES, MAX_ITERS, trans)
    return res["transformation"], res["information"]


def _trajectory(x, name: str) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: no GPU (pointdsc_amd has no CPU path)")
        x = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    if not torch.is_tensor(x):
        raise TypeError(f"{name} must be a numpy array or a tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    if x.dim() != 2 or x.shape[0] != 3 or x.shape[1] < 1:
        raise ValueError(f"{name} must be [3,num_frag], got {tuple(x.shape)}")
    return x.float().T[None].contiguous()


def align(model_traj, data_traj) -> Tuple[torch.Tensor, torch.Tensor]:
    """multiway/test_multi_ate.py:31-51: the rigid motion that aligns trajectory ``model_traj`` onto ``data_traj`` (both
    [3,num_frag], as the driver passes them: numpy arrays are moved to the current GPU, tensors must be there already)
    -> (trans [4,4] fp32, per-fragment error in cm [num_frag]), both on the device."""
    model, data = _trajectory(model_traj, "model_traj"), _trajectory(data_traj, "data_traj")
    if model.shape != data.shape or model.device != data.device:
        raise ValueError(f"trajectories differ: {tuple(model.shape)} on {model.device} against {tuple(data.shape)} on {data.device}")
    trans = ops.rigid_transform_3d(model, data)                                # :44
    aligned = model @ trans[:, :3, :3].transpose(1, 2) + trans[:, None, :3, 3]  # utils/SE3.py transform
    err = torch.norm(aligned - data, dim=-1)[0] * 100.0                        # m -> cm
    return trans[0], err


__all__: List[str] = ["information_matrix", "voxel_down_sample", "loop_closure_edge", "overlap_gate", "multi_scale_icp",
                      "local_refinement", "align", "EDGE_DISTANCE", "MIN_OVERLAP", "VOXEL_SIZES", "MAX_ITERS"]
