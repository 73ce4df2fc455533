"""The multiway driver's edge step and pose-graph optimisation on the device: what
``multiway/test_multi_ate.py`` does around ``model(data)`` with open3d on the host -- the edge's information matrix and overlap gate
(:141-149), multi-scale ICP of the odometry edges (:54-83), the node chain (:129-130), ``o3d.registration.global_optimization``
(:166-174, :217-224: Levenberg-Marquardt with the line process and edge pruning, ``global_optimization`` here) and the trajectory
alignment of its ATE (:31-51).

The arithmetic runs in libpointdsc_hip.so (``pdsc_information_matrix``, ``pdsc_voxel_keys`` / ``pdsc_voxel_means``,
``pdsc_icp_refine``, ``pdsc_posegraph_nodes``, ``pdsc_global_optimization``); nothing here reads a device value on the host, so per-pair point counts stay on the device from one
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


# ---------------------------------------------------------------------------------------------------------------------------
# pose graph: multiway/test_multi_ate.py:129-130 and :166-174
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_KEYS = ("source", "target", "transformation", "information", "uncertain")
MAX_NODES = 128                                     # PDSC_POSEGRAPH_MAX_NODES
RECORD_NAMES = ("status", "pass1_iterations", "pass1_solves", "pass1_objective", "pass1_w", "pass2_iterations", "pass2_solves",
                "pass2_objective", "pass2_w", "edges_in", "edges_after_pass1", "edges_out")


def _graph_edges(edges, name: str = "edges") -> Tuple[List[Dict[str, torch.Tensor]], bool]:
    """One graph's edges (a dict with the EDGE_KEYS, or a tuple in that order) or a list of them -> (list of checked dicts, single)."""
    single = isinstance(edges, dict) or (isinstance(edges, (tuple, list)) and len(edges) == 5 and torch.is_tensor(edges[0]))
    graphs = [edges] if single else list(edges)
    if not graphs:
        raise ValueError(f"{name}: no graph")
    out = []
    for gi, e in enumerate(graphs):
        if not isinstance(e, dict):
            if not (isinstance(e, (tuple, list)) and len(e) == 5):
                raise TypeError(f"{name}[{gi}] must be a dict with the keys {EDGE_KEYS} or a tuple in that order")
            e = dict(zip(EDGE_KEYS, e))
        missing = [k for k in EDGE_KEYS if k not in e]
        if missing:
            raise ValueError(f"{name}[{gi}] lacks {missing}")
        for k in EDGE_KEYS:
            if not torch.is_tensor(e[k]):
                raise TypeError(f"{name}[{gi}][{k!r}] must be a tensor")
        E = int(e["source"].shape[0]) if e["source"].dim() == 1 else -1
        if E < 0 or tuple(e["target"].shape) != (E,) or tuple(e["uncertain"].shape) != (E,):
            raise ValueError(f"{name}[{gi}]: source, target and uncertain must be [E]")
        if tuple(e["transformation"].shape) != (E, 4, 4) or tuple(e["information"].shape) != (E, 6, 6):
            raise ValueError(f"{name}[{gi}]: transformation must be [E,4,4] and information [E,6,6] for E = {E}, got "
                             f"{tuple(e['transformation'].shape)} and {tuple(e['information'].shape)}")
        if e["transformation"].dtype not in (torch.float32, torch.float64) or e["information"].dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{name}[{gi}]: transformation and information must be fp32 or fp64 (fp32 is widened exactly)")
        if e["source"].dtype not in (torch.int32, torch.int64) or e["target"].dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name}[{gi}]: source and target must be int32 or int64")
        out.append(e)
    return out, single


def _edges_on_device(graphs, name: str = "edges") -> None:
    for gi, e in enumerate(graphs):
        for k in EDGE_KEYS:
            if not e[k].is_cuda:
                raise RuntimeError(f"{name}[{gi}][{k!r}] must live on the GPU (pointdsc_amd has no CPU path)")


def _flat_edges(graphs: List[Dict[str, torch.Tensor]], dev) -> Dict[str, torch.Tensor]:
    cat = lambda k, dt: torch.cat([g[k].to(dt).flatten(1) if g[k].dim() > 1 else g[k].to(dt) for g in graphs])  # noqa: E731
    flat = {"source": cat("source", torch.int32), "target": cat("target", torch.int32), "X": cat("transformation", torch.float64),
            "info": cat("information", torch.float64), "uncertain": cat("uncertain", torch.uint8)}
    if flat["source"].numel() == 0:                 # no edge at all: the library still wants non-null arrays
        flat = {"source": torch.zeros(1, dtype=torch.int32, device=dev), "target": torch.zeros(1, dtype=torch.int32, device=dev),
                "X": torch.zeros(1, 16, dtype=torch.float64, device=dev), "info": torch.zeros(1, 36, dtype=torch.float64, device=dev),
                "uncertain": torch.zeros(1, dtype=torch.uint8, device=dev)}
    return {k: v.contiguous() for k, v in flat.items()}


def _offsets(counts: List[int], dev) -> torch.Tensor:
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev, non_blocking=True)


def _edge_masks(edge_mask, graphs, single: bool, dev) -> Optional[torch.Tensor]:
    if edge_mask is None:
        return None
    masks = [edge_mask] if single and torch.is_tensor(edge_mask) else list(edge_mask)
    if len(masks) != len(graphs):
        raise ValueError(f"edge_mask: {len(masks)} masks for {len(graphs)} graphs")
    for m, g in zip(masks, graphs):
        if not torch.is_tensor(m) or tuple(m.shape) != tuple(g["source"].shape):
            raise ValueError(f"edge_mask must be [E] = {tuple(g['source'].shape)} per graph")
        if not m.is_cuda:
            raise RuntimeError("edge_mask must live on the GPU (pointdsc_amd has no CPU path)")
    flat = torch.cat([(m != 0).to(torch.uint8) for m in masks])
    return flat.contiguous() if flat.numel() else torch.ones(1, dtype=torch.uint8, device=dev)


@_on_device
def pose_graph_nodes(edges, num_nodes=None, edge_mask=None):
    """The driver's node chain (multiway/test_multi_ate.py:129-130, :202-203) of one graph or a list of graphs: node 0 = identity,
    and per certain edge (in order; with ``edge_mask`` only those it keeps) ``odometry = X @ odometry``, next node =
    ``inv(odometry)`` under INVERSE_RULE.  ``num_nodes`` (int, or one per graph): the number of fragments (counting the certain
    edges would read the device).  Nodes the chain does not reach are NaN.  -> [F,4,4] fp64 on the device (or a list)."""
    lib = _lib.load()
    graphs, single = _graph_edges(edges)
    if num_nodes is None:
        raise ValueError("num_nodes is required: the number of fragments")
    _edges_on_device(graphs)
    counts = [int(num_nodes)] * len(graphs) if isinstance(num_nodes, (int, np.integer)) else [int(n) for n in num_nodes]
    if len(counts) != len(graphs) or min(counts) < 1:
        raise ValueError(f"num_nodes: need one positive count per graph, got {counts} for {len(graphs)} graphs")
    dev = graphs[0]["source"].device
    flat = _flat_edges(graphs, dev)
    live = _edge_masks(edge_mask, graphs, single, dev)
    ecounts = [int(g["source"].shape[0]) for g in graphs]
    nodes = torch.empty(sum(counts), 4, 4, dtype=torch.float64, device=dev)
    node_offset, edge_offset = _offsets(counts, dev), _offsets(ecounts, dev)       # both alive until the launch is enqueued
    _lib.check(lib.pdsc_posegraph_nodes(_p(flat["X"]), _p(flat["uncertain"]), _p(live), _p(node_offset), _p(edge_offset), _p(nodes),
                                        len(graphs), sum(counts), sum(ecounts), _stream()), "pdsc_posegraph_nodes")
    parts = list(torch.split(nodes, counts))
    return parts[0] if single else parts


@_on_device
def global_optimization(nodes, edges, max_correspondence_distance: float = EDGE_DISTANCE, edge_prune_threshold: float = 0.25,
                        preference_loop_closure: float = 20.0, reference_node: int = 0, edge_mask=None) -> Dict[str, object]:
    """``o3d.registration.global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(),
    GlobalOptimizationConvergenceCriteria(), GlobalOptimizationOption(...))`` (multiway/test_multi_ate.py:166-174) of one graph or
    a list of graphs, on the device (``pdsc_global_optimization``: the contract is in include/pointdsc_hip.h).

    ``nodes`` [F,4,4] (fragment -> world; fp32 or fp64); ``edges``: a dict with ``source`` / ``target`` [E] (int), ``transformation``
    [E,4,4] (the fp32 ``final_trans`` of the forward or the fp64 ``transformation_f64`` of the ICP; fp32 is widened exactly),
    ``information`` [E,6,6] and ``uncertain`` [E] (bool), or a tuple in that order; or lists of both.  ``edge_mask`` [E] (bool;
    ``loop_closure_edge(...)["keep"]`` goes in directly): edges that take part -- pruning is a mask, nothing is compacted.

    Returns ``nodes`` [F,4,4] fp64, ``confidence`` [E] fp64, ``keep`` [E] bool (the edges that are live at the end) and ``record``
    [12] fp64 (``RECORD_NAMES``: status, per pass outer iterations / solves / objective / w, edge counts), all on the device --
    nothing is read on the host; lists of per-graph tensors (``record`` [G,12]) when lists were given.  An invalid graph (status 1)
    has NaN nodes."""
    for name, v in (("max_correspondence_distance", max_correspondence_distance), ("edge_prune_threshold", edge_prune_threshold),
                    ("preference_loop_closure", preference_loop_closure)):
        if not math.isfinite(float(v)):
            raise ValueError(f"{name} must be finite, got {v}")
    graphs, single = _graph_edges(edges)
    node_list = [nodes] if torch.is_tensor(nodes) else list(nodes)
    if torch.is_tensor(nodes) != single or len(node_list) != len(graphs):
        raise ValueError(f"nodes and edges must both be one graph or lists of the same length, got {len(node_list)} and {len(graphs)}")
    for gi, nd in enumerate(node_list):
        if not torch.is_tensor(nd) or nd.dim() != 3 or tuple(nd.shape[1:]) != (4, 4) or nd.shape[0] < 1:
            raise ValueError(f"nodes[{gi}] must be [F,4,4] with F >= 1")
        if nd.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"nodes[{gi}] must be fp32 or fp64")
    _edges_on_device(graphs)
    for gi, nd in enumerate(node_list):
        if not nd.is_cuda:
            raise RuntimeError(f"nodes[{gi}] must live on the GPU (pointdsc_amd has no CPU path)")
    fcounts = [int(nd.shape[0]) for nd in node_list]
    if max(fcounts) > MAX_NODES:
        raise ValueError(f"a graph of {max(fcounts)} nodes is beyond PDSC_POSEGRAPH_MAX_NODES = {MAX_NODES}")
    if not (0 <= int(reference_node) < min(fcounts)):
        raise ValueError(f"reference_node {reference_node} outside [0, {min(fcounts)})")
    dev = node_list[0].device
    call = _posegraph_call(node_list, graphs, _edge_masks(edge_mask, graphs, single, dev), float(max_correspondence_distance),
                           float(edge_prune_threshold), float(preference_loop_closure), int(reference_node))
    _posegraph_launch(call)
    fcounts, ecounts = call["fcounts"], call["ecounts"]
    nodes_out = call["nodes_out"].view(-1, 4, 4)
    conf, keep = call["confidence"][:sum(ecounts)], call["keep"][:sum(ecounts)].bool()
    if single:
        return {"nodes": nodes_out, "confidence": conf, "keep": keep, "record": call["record"][0]}
    return {"nodes": list(torch.split(nodes_out, fcounts)), "confidence": list(torch.split(conf, ecounts)),
            "keep": list(torch.split(keep, ecounts)), "record": call["record"]}


def _posegraph_call(node_list, graphs, live, max_distance: float, prune_threshold: float, preference: float, reference: int,
                    ticks: bool = False):
    """Every buffer of one ``pdsc_global_optimization`` call (inputs flattened, offsets, outputs, workspace), allocated once:
    ``_posegraph_launch`` then only enqueues the kernel, so that it can be captured into a graph and replayed.  ``ticks``: also
    the [G,3] int64 array of the kernel's own clock readings (tools/posegraph_bench.py)."""
    lib = _lib.load()
    dev = node_list[0].device
    fcounts = [int(nd.shape[0]) for nd in node_list]
    ecounts = [int(g["source"].shape[0]) for g in graphs]
    call = _flat_edges(graphs, dev)
    call["nodes_in"] = torch.cat([nd.to(torch.float64).reshape(-1, 16) for nd in node_list]).contiguous()
    call["nodes_out"] = torch.empty_like(call["nodes_in"])
    call["confidence"] = torch.empty(max(sum(ecounts), 1), dtype=torch.float64, device=dev)
    call["keep"] = torch.empty(max(sum(ecounts), 1), dtype=torch.uint8, device=dev)
    call["record"] = torch.empty(len(graphs), len(RECORD_NAMES), dtype=torch.float64, device=dev)
    call["ticks"] = torch.zeros(len(graphs), 3, dtype=torch.int64, device=dev) if ticks else None
    call["ws_bytes"] = int(lib.pdsc_posegraph_workspace_bytes(len(graphs), max(fcounts), max(ecounts)))
    call["ws"] = torch.empty(call["ws_bytes"], dtype=torch.uint8, device=dev)
    call["node_offset"], call["edge_offset"] = _offsets(fcounts, dev), _offsets(ecounts, dev)
    call.update(live=live, fcounts=fcounts, ecounts=ecounts, options=(max_distance, prune_threshold, preference, reference))
    return call


def _posegraph_launch(c) -> None:
    lib = _lib.load()
    d, thr, pref, ref = c["options"]
    _lib.check(lib.pdsc_global_optimization(_p(c["nodes_in"]), _p(c["source"]), _p(c["target"]), _p(c["X"]), _p(c["info"]),
                                            _p(c["uncertain"]), _p(c["live"]), _p(c["node_offset"]), _p(c["edge_offset"]), d, thr, pref,
                                            ref, _p(c["nodes_out"]), _p(c["confidence"]), _p(c["keep"]), _p(c["record"]), _p(c["ticks"]), _p(c["ws"]),
                                            c["ws_bytes"], len(c["fcounts"]), max(c["fcounts"]), max(c["ecounts"]), sum(c["fcounts"]),
                                            sum(c["ecounts"]), _stream()), "pdsc_global_optimization")


__all__: List[str] = ["information_matrix", "voxel_down_sample", "loop_closure_edge", "overlap_gate", "multi_scale_icp",
                      "local_refinement", "align", "pose_graph_nodes", "global_optimization", "EDGE_DISTANCE", "MIN_OVERLAP",
                      "VOXEL_SIZES", "MAX_ITERS", "RECORD_NAMES"]
