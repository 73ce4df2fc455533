"""The evaluation's optional ICP post-step on the device (the open3d hand-off of SURVEY.md section 8 f-4).

``icp_refine`` has the signature and meaning of the reference's ``evaluation/benchmark_utils.py:40-56`` (open3d 0.9
``registration_icp``, point-to-point, max_correspondence_distance 0.10, default criteria); ``registration_icp`` exposes
the criteria and the result record.  The loop runs in libpointdsc_hip.so (``pdsc_icp_refine``, csrc/icp.hip): one launch per
call, no host synchronisation, so it can sit inside the timed model window and inside a captured graph.  GPU only.

Inputs are ``[bs,N,3]`` tensors (every pair has N points) or lists of per-pair ``[n_b,3]`` / ``[1,n_b,3]`` tensors (a ragged
batch: padded to the longest pair, per-pair counts on the device).  Source and target counts may differ.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Union

import torch

from . import _lib
from .ops import _chk, _on_device, _p, _stream

Points = Union[torch.Tensor, Sequence[torch.Tensor]]

# open3d 0.9 ICPConvergenceCriteria() defaults, as the reference's icp_refine uses them
RELATIVE_FITNESS = 1e-6
RELATIVE_RMSE = 1e-6
MAX_ITERATION = 30
MAX_CORRESPONDENCE_DISTANCE = 0.10


def _as_batch(x: Points, name: str):
    """-> (padded [bs,n_max,3] fp32 tensor, per-pair counts list, device counts tensor or None)."""
    if torch.is_tensor(x):
        if x.dim() != 3 or x.shape[-1] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"{name} must be [bs,N,3] with bs, N >= 1, got {tuple(x.shape)}")
        return _chk(x, name), [int(x.shape[1])] * int(x.shape[0]), None
    parts = list(x)
    if not parts:
        raise ValueError(f"{name}: empty list of pairs")
    rows = []
    for i, t in enumerate(parts):
        if not torch.is_tensor(t):
            raise TypeError(f"{name}[{i}] is not a tensor")
        if t.dim() == 3 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 2 or t.shape[-1] != 3 or t.shape[0] < 1:
            raise ValueError(f"{name}[{i}] must be [n,3] or [1,n,3] with n >= 1, got {tuple(t.shape)}")
        rows.append(_chk(t, f"{name}[{i}]"))
    dev = rows[0].device
    if any(r.device != dev for r in rows):
        raise ValueError(f"{name}: every pair must live on the same device")
    counts = [int(r.shape[0]) for r in rows]
    n_max = max(counts)
    out = torch.zeros(len(rows), n_max, 3, device=dev, dtype=torch.float32)
    for i, r in enumerate(rows):
        out[i, :counts[i]] = r
    return out, counts, torch.tensor(counts, dtype=torch.int32).to(dev, non_blocking=True)


def _counts(counts, bs: int, dev, name: str):
    """Per-pair point counts that are already on the device ([bs] int32): what keeps a chain of calls free of host reads."""
    if counts is None:
        return None
    if not torch.is_tensor(counts):
        raise TypeError(f"{name} must be a tensor")
    counts = _chk(counts, name, torch.int32)
    if tuple(counts.shape) != (bs,) or counts.device != dev:
        raise ValueError(f"{name} must be [{bs}] int32 on {dev}, got {tuple(counts.shape)} on {counts.device}")
    return counts


def _pair_batches(source: Points, target: Points, source_counts=None, target_counts=None):
    """-> (src [bs,Ns,3], tgt [bs,Nt,3], ns_dev, nt_dev): both per-pair count tensors, or None for both when every pair is full."""
    src, _, ns_dev = _as_batch(source, "source")
    tgt, _, nt_dev = _as_batch(target, "target")
    bs = src.shape[0]
    if tgt.shape[0] != bs:
        raise ValueError(f"source has {bs} pairs, target {tgt.shape[0]}")
    if src.device != tgt.device:
        raise ValueError("source and target must live on the same device")
    dev = src.device
    if source_counts is not None:
        if ns_dev is not None:
            raise ValueError("source_counts goes with a padded [bs,N,3] tensor, not with a list of pairs")
        ns_dev = _counts(source_counts, bs, dev, "source_counts")
    if target_counts is not None:
        if nt_dev is not None:
            raise ValueError("target_counts goes with a padded [bs,N,3] tensor, not with a list of pairs")
        nt_dev = _counts(target_counts, bs, dev, "target_counts")
    if ns_dev is None and nt_dev is not None:
        ns_dev = torch.full((bs,), src.shape[1], dtype=torch.int32, device=dev)
    if nt_dev is None and ns_dev is not None:
        nt_dev = torch.full((bs,), tgt.shape[1], dtype=torch.int32, device=dev)
    return src, tgt, ns_dev, nt_dev


def _as_poses(T: torch.Tensor, bs: int, name: str) -> torch.Tensor:
    if not torch.is_tensor(T):
        raise TypeError(f"{name} must be a tensor")
    T = _chk(T, name)
    if T.shape == (4, 4):
        T = T.expand(bs, 4, 4)
    if tuple(T.shape) != (bs, 4, 4):
        raise ValueError(f"{name} must be [4,4] or [{bs},4,4], got {tuple(T.shape)}")
    return T.contiguous()


@_on_device
def registration_icp(source: Points, target: Points, init: torch.Tensor,
                     max_correspondence_distance: float = MAX_CORRESPONDENCE_DISTANCE,
                     relative_fitness: float = RELATIVE_FITNESS, relative_rmse: float = RELATIVE_RMSE,
                     max_iteration: int = MAX_ITERATION, source_counts: Optional[torch.Tensor] = None,
                     target_counts: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """open3d 0.9 ``registration.registration_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationPointToPoint(), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))``
    for every pair of the batch.  ``init`` [bs,4,4] or [4,4] (shared by all pairs), fp32.  ``source_counts`` / ``target_counts``
    ([bs] int32 on the device) give the valid rows of padded ``[bs,N,3]`` inputs without a host read.

    Returns a dict of device tensors: ``transformation`` [bs,4,4] fp32, ``transformation_f64`` [bs,4,4] fp64,
    ``fitness`` [bs] fp64, ``inlier_rmse`` [bs] fp64, ``num_correspondences`` [bs] int32 (the final correspondence set),
    ``iterations`` [bs] int32.  A non-finite init or point gives a NaN transformation and 0 iterations;
    ``max_correspondence_distance <= 0`` returns init (as open3d does)."""
    lib = _lib.load()
    if math.isnan(float(max_correspondence_distance)):
        raise ValueError("max_correspondence_distance is NaN")
    if math.isnan(float(relative_fitness)) or math.isnan(float(relative_rmse)):
        raise ValueError("relative_fitness / relative_rmse must not be NaN")
    if int(max_iteration) < 0:
        raise ValueError(f"max_iteration must be >= 0, got {max_iteration}")
    src, tgt, ns_dev, nt_dev = _pair_batches(source, target, source_counts, target_counts)
    bs, dev = src.shape[0], src.device
    init = _as_poses(init, bs, "init")
    Ns, Nt = int(src.shape[1]), int(tgt.shape[1])
    ws_bytes = int(lib.pdsc_icp_workspace_bytes(bs, Ns, Nt))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out32 = torch.empty(bs, 4, 4, dtype=torch.float32, device=dev)
    out64 = torch.empty(bs, 4, 4, dtype=torch.float64, device=dev)
    fitness = torch.empty(bs, dtype=torch.float64, device=dev)
    rmse = torch.empty(bs, dtype=torch.float64, device=dev)
    ncorr = torch.empty(bs, dtype=torch.int32, device=dev)
    iters = torch.empty(bs, dtype=torch.int32, device=dev)
    _lib.check(lib.pdsc_icp_refine(_p(src), _p(tgt), _p(init), _p(ns_dev), _p(nt_dev), float(max_correspondence_distance),
                                   float(relative_fitness), float(relative_rmse), int(max_iteration), _p(out32), _p(out64),
                                   _p(fitness), _p(rmse), _p(ncorr), _p(iters), _p(ws), ws_bytes, bs, Ns, Nt, _stream()),
               "pdsc_icp_refine")
    return {"transformation": out32, "transformation_f64": out64, "fitness": fitness, "inlier_rmse": rmse,
            "num_correspondences": ncorr, "iterations": iters,
            "criteria": {"relative_fitness": float(relative_fitness), "relative_rmse": float(relative_rmse),
                         "max_iteration": int(max_iteration)}}


def icp_refine(src_keypts: Points, tgt_keypts: Points, pred_trans: torch.Tensor,
               max_correspondence_distance: float = MAX_CORRESPONDENCE_DISTANCE) -> torch.Tensor:
    """evaluation/benchmark_utils.py:40-56: refine ``pred_trans`` [bs,4,4] by point-to-point ICP from the correspondence
    endpoints ``src_keypts`` onto ``tgt_keypts`` ([bs,N,3] or lists of per-pair tensors) -> [bs,4,4] fp32 on their device."""
    return registration_icp(src_keypts, tgt_keypts, pred_trans, max_correspondence_distance)["transformation"]


__all__: List[str] = ["icp_refine", "registration_icp", "RELATIVE_FITNESS", "RELATIVE_RMSE", "MAX_ITERATION",
                      "MAX_CORRESPONDENCE_DISTANCE"]
