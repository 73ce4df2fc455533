"""FPFH descriptors on the device: what the reference's FPFH track gets from open3d.

``fpfh_descriptors`` is the recipe of ``misc/cal_fpfh.py:21-26`` on an already down-sampled cloud -- ``estimate_normals`` with
``KDTreeSearchParamHybrid(radius=2 voxel, max_nn=30)``, ``compute_fpfh_feature`` with ``KDTreeSearchParamHybrid(radius=5 voxel,
max_nn=100)`` -- followed by the demo's normalisation ``f / (|f|_2 + 1e-6)`` (``demo_registration.py:43``): fp32 [n,33]
descriptors ready for ``correspondences.build_correspondences``.  The stages are exposed one by one (``hybrid_neighbours``,
``estimate_normals``, ``compute_fpfh_feature``).  Everything runs in libpointdsc_hip.so (csrc/fpfh.hip), fp64, without a host
synchronisation, so the calls can sit inside a captured graph.  GPU only.

Inputs are ``[bs,N,3]`` tensors (with optional per-cloud ``counts`` [bs] int32 on the device) or lists of per-cloud ``[n_b,3]``
tensors (a ragged batch: padded to the longest cloud), as in ``icp.py`` and ``multiway.py``.  Outputs are padded the same way: rows
beyond a cloud's count are zero.  A cloud with a non-finite point gets NaN rows (neighbour count -1).

Three named rules, stated in include/pointdsc_hip.h: FLANN_RADIUS_RULE (``d2 < float32(r * r)``), COVARIANCE_ORDER_RULE (cumulants
summed in ascending neighbour index order), NORMAL_SIGN_RULE (normals point towards ``viewpoint``, default the origin).

``extract_fpfh_features`` is the demo's own recipe (``demo_registration.py:37-44``) on RAW clouds of any
size: normals on the raw cloud, ``voxel_down_sample_with_normals`` (open3d's voxel step, which averages the normals of a voxel:
VOXEL_NORMAL_RULE, CAPACITY_RULE), the descriptor on the down-sampled cloud with those normals.  ``path`` selects the kernels in front
of the descriptor: "auto", "one" (one workgroup per cloud) or "many" (many workgroups per cloud); the results are bit-identical.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .icp import Points, _as_batch, _counts
from .ops import _chk, _on_device, _p, _stream

FPFH_DIM = 33
MAX_NN_LIMIT = 128
# misc/cal_fpfh.py:21-26
NORMAL_RADIUS_VOXELS = 2.0
NORMAL_MAX_NN = 30
FEATURE_RADIUS_VOXELS = 5.0
FEATURE_MAX_NN = 100


def _cloud_batch(points: Points, counts):
    pts, _, n_dev = _as_batch(points, "points")
    if counts is not None:
        if n_dev is not None:
            raise ValueError("counts goes with a padded [bs,N,3] tensor, not with a list of clouds")
        n_dev = _counts(counts, int(pts.shape[0]), pts.device, "counts")
    return pts, n_dev


def _radius(r, name: str) -> float:
    r = float(r)
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError(f"{name} must be positive and finite, got {r}")
    return r


def _max_nn(k, name: str) -> int:
    k = int(k)
    if not 1 <= k <= MAX_NN_LIMIT:
        raise ValueError(f"{name} must be in 1 .. {MAX_NN_LIMIT}, got {k}")
    return k


def _viewpoint(viewpoint):
    """-> a ctypes double[3] (read by the library before the call returns) or None for the origin."""
    if viewpoint is None:
        return None
    v = [float(x) for x in (viewpoint.tolist() if torch.is_tensor(viewpoint) else viewpoint)]
    if len(v) != 3 or not all(math.isfinite(x) for x in v):
        raise ValueError(f"viewpoint must be 3 finite numbers, got {viewpoint}")
    return (C.c_double * 3)(*v)


PATHS = {"auto": 0, "one": 1, "many": 2}             # PDSC_PATH_AUTO / _ONE_WORKGROUP / _MANY


def _path(path) -> int:
    if path not in PATHS:
        raise ValueError(f"path must be one of {sorted(PATHS)}, got {path!r}")
    return PATHS[path]


def _lists(lib, pts, n_dev, radius: float, max_nn: int, want_d2: bool = True, path: int = 0):
    bs, n, dev = int(pts.shape[0]), int(pts.shape[1]), pts.device
    ws_bytes = int(lib.pdsc_hybrid_neighbours_workspace_bytes(bs, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    idx = torch.empty(bs, n, max_nn, dtype=torch.int32, device=dev)
    d2 = torch.empty(bs, n, max_nn, dtype=torch.float64, device=dev) if want_d2 else None
    count = torch.empty(bs, n, dtype=torch.int32, device=dev)
    _lib.check(lib.pdsc_cloud_neighbours(_p(pts), _p(n_dev), radius, max_nn, _p(idx), _p(d2), _p(count), _p(ws), ws_bytes, bs, n, path,
                                         _stream()), "pdsc_cloud_neighbours")
    return idx, d2, count


@_on_device
def hybrid_neighbours(points: Points, radius: float, max_nn: int, counts: Optional[torch.Tensor] = None,
                      path: str = "auto") -> Dict[str, torch.Tensor]:
    """open3d ``KDTreeFlann.search_hybrid_vector_3d(p, radius, max_nn)`` for every point of every cloud: the at most ``max_nn``
    (<= 128) nearest points of the same cloud with fp64 ``d2 < float32(radius * radius)``, ascending by (d2, index); the point
    itself is included.  Returns ``idx`` [bs,N,max_nn] int32 (-1 beyond the count), ``d2`` [bs,N,max_nn] fp64, ``count`` [bs,N]
    int32 (0 for padding rows, -1 for every row of a cloud with a non-finite point).  ``path``: how the cell grid is built ("auto",
    "one" workgroup per cloud, "many"); the lists do not depend on it."""
    lib = _lib.load()
    radius, max_nn, path = _radius(radius, "radius"), _max_nn(max_nn, "max_nn"), _path(path)
    pts, n_dev = _cloud_batch(points, counts)
    idx, d2, count = _lists(lib, pts, n_dev, radius, max_nn, path=path)
    return {"idx": idx, "d2": d2, "count": count}


@_on_device
def estimate_normals(points: Points, radius: float, max_nn: int = NORMAL_MAX_NN, viewpoint=None,
                     counts: Optional[torch.Tensor] = None, path: str = "auto") -> torch.Tensor:
    """open3d 0.9 ``estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))`` followed by
    ``orient_normals_towards_camera_location(viewpoint)`` (NORMAL_SIGN_RULE; default the origin) -> [bs,N,3] fp64 unit normals;
    (0, 0, 1) for a point with fewer than 3 neighbours."""
    lib = _lib.load()
    radius, max_nn, vp, path = _radius(radius, "radius"), _max_nn(max_nn, "max_nn"), _viewpoint(viewpoint), _path(path)
    pts, n_dev = _cloud_batch(points, counts)
    bs, n = int(pts.shape[0]), int(pts.shape[1])
    idx, _, count = _lists(lib, pts, n_dev, radius, max_nn, want_d2=False, path=path)
    normals = torch.empty(bs, n, 3, dtype=torch.float64, device=pts.device)
    _lib.check(lib.pdsc_estimate_normals(_p(pts), _p(n_dev), _p(idx), _p(count), max_nn, vp, _p(normals), bs, n, _stream()),
               "pdsc_estimate_normals")
    return normals


@_on_device
def compute_fpfh_feature(points: Points, radius: float, max_nn: int = FEATURE_MAX_NN, normals: Optional[torch.Tensor] = None,
                         normal_radius: Optional[float] = None, normal_max_nn: int = NORMAL_MAX_NN, viewpoint=None,
                         counts: Optional[torch.Tensor] = None, path: str = "auto") -> Dict[str, torch.Tensor]:
    """open3d 0.9 ``registration.compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn))``.

    With ``normals`` ([bs,N,3] fp64 on the device, e.g. from ``estimate_normals``) the stages run one by one and the result also
    holds ``spfh``; without, ``normal_radius`` is required and the whole chain runs in one library call (``pdsc_fpfh``).
    Returns ``fpfh`` [bs,N,33] fp64 (open3d's feature, transposed: one row per point), ``desc`` [bs,N,33] fp32
    (``fpfh / (|fpfh|_2 + 1e-6)``), ``normals`` [bs,N,3] fp64.  ``path`` (with ``normals`` only; ``pdsc_fpfh`` chooses by itself): how
    the cell grid of the lists is built, as in ``hybrid_neighbours``."""
    lib = _lib.load()
    radius, max_nn, path = _radius(radius, "radius"), _max_nn(max_nn, "max_nn"), _path(path)
    if normals is None and normal_radius is None:
        raise ValueError("compute_fpfh_feature needs normals or a normal_radius to estimate them with")
    if normals is None and path != PATHS["auto"]:
        raise ValueError("path goes with normals: without them the whole chain is one pdsc_fpfh call, which chooses by itself")
    pts, n_dev = _cloud_batch(points, counts)
    bs, n, dev = int(pts.shape[0]), int(pts.shape[1]), pts.device
    fpfh = torch.empty(bs, n, FPFH_DIM, dtype=torch.float64, device=dev)
    desc = torch.empty(bs, n, FPFH_DIM, dtype=torch.float32, device=dev)
    if normals is None:
        normal_radius, normal_max_nn, vp = _radius(normal_radius, "normal_radius"), _max_nn(normal_max_nn, "normal_max_nn"), _viewpoint(viewpoint)
        normals = torch.empty(bs, n, 3, dtype=torch.float64, device=dev)
        ws_bytes = int(lib.pdsc_fpfh_workspace_bytes(bs, n, normal_max_nn, max_nn))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.pdsc_fpfh(_p(pts), _p(n_dev), normal_radius, normal_max_nn, radius, max_nn, vp, _p(fpfh), _p(desc), _p(normals),
                                 _p(ws), ws_bytes, bs, n, _stream()), "pdsc_fpfh")
        return {"fpfh": fpfh, "desc": desc, "normals": normals}
    if not torch.is_tensor(normals):
        raise TypeError("normals must be a tensor")
    normals = _chk(normals, "normals", torch.float64)
    if tuple(normals.shape) != (bs, n, 3) or normals.device != dev:
        raise ValueError(f"normals must be [{bs},{n},3] fp64 on {dev}, got {tuple(normals.shape)} on {normals.device}")
    idx, d2, count = _lists(lib, pts, n_dev, radius, max_nn, path=path)
    spfh = torch.empty(bs, n, FPFH_DIM, dtype=torch.float64, device=dev)
    _lib.check(lib.pdsc_spfh(_p(pts), _p(n_dev), _p(normals), _p(idx), _p(count), max_nn, _p(spfh), bs, n, _stream()), "pdsc_spfh")
    _lib.check(lib.pdsc_fpfh_from_spfh(_p(spfh), _p(n_dev), _p(idx), _p(d2), _p(count), max_nn, _p(fpfh), _p(desc), bs, n, _stream()),
               "pdsc_fpfh_from_spfh")
    return {"fpfh": fpfh, "desc": desc, "normals": normals, "spfh": spfh}


@_on_device
def fpfh_descriptors(points: Points, voxel_size: float, counts: Optional[torch.Tensor] = None, viewpoint=None) -> torch.Tensor:
    """misc/cal_fpfh.py:21-26 + demo_registration.py:43 on clouds already down-sampled at ``voxel_size``: [bs,N,33] fp32
    L2-normalised FPFH descriptors (one ``pdsc_fpfh`` call for the batch)."""
    v = _radius(voxel_size, "voxel_size")
    return compute_fpfh_feature(points, FEATURE_RADIUS_VOXELS * v, FEATURE_MAX_NN, normal_radius=NORMAL_RADIUS_VOXELS * v,
                                normal_max_nn=NORMAL_MAX_NN, viewpoint=viewpoint, counts=counts)["desc"]


def _capacity(capacity) -> Optional[int]:
    if capacity is None:
        return None
    c = int(capacity)
    if not 1 <= c <= (1 << 24):
        raise ValueError(f"capacity must be in 1 .. 2^24, got {capacity}")
    return c


def _voxel_with_normals(lib, pts, n_dev, normals, v: float, cap: Optional[int], renormalize: bool, path: int):
    """keys -> stable sort -> means with normals; cap None: sized exactly (one host read of the counts)."""
    bs, n, dev = int(pts.shape[0]), int(pts.shape[1]), pts.device
    ws_bytes = int(lib.pdsc_cloud_voxel_workspace_bytes(bs, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    keys = torch.empty(bs, n, dtype=torch.int64, device=dev)
    _lib.check(lib.pdsc_cloud_voxel_keys(_p(pts), _p(n_dev), v, _p(keys), _p(ws), ws_bytes, bs, n, path, _stream()),
               "pdsc_cloud_voxel_keys")
    sorted_keys, perm = torch.sort(keys, dim=1, stable=True)        # plumbing; keys and means are the library's
    rows = n if cap is None else cap
    out = torch.empty(bs, rows, 3, dtype=torch.float32, device=dev)
    out_n = torch.empty(bs, rows, 3, dtype=torch.float64, device=dev)
    out_counts = torch.empty(bs, dtype=torch.int32, device=dev)
    _lib.check(lib.pdsc_cloud_voxel_means(_p(pts), _p(normals), _p(sorted_keys.contiguous()), _p(perm.contiguous()), _p(out), _p(out_n),
                                          _p(out_counts), rows, int(bool(renormalize)), _p(ws), ws_bytes, bs, n, path, _stream()),
               "pdsc_cloud_voxel_means")
    if cap is None:
        exact = max(1, int(out_counts.max().item()))                # the one host synchronisation of capacity=None
        out, out_n = out[:, :exact].contiguous(), out_n[:, :exact].contiguous()
    return out, out_n, out_counts


@_on_device
def voxel_down_sample_with_normals(points: Points, normals: torch.Tensor, voxel_size: float, counts: Optional[torch.Tensor] = None,
                                   capacity: Optional[int] = None, renormalize: bool = False,
                                   path: str = "auto") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """open3d ``PointCloud.voxel_down_sample(voxel_size)`` of clouds that carry normals: ``multiway.voxel_down_sample`` (same
    voxels, same order, bit-equal mean points) plus the fp64 mean normal of every voxel (VOXEL_NORMAL_RULE: not renormalised;
    ``renormalize=True`` divides by the norm and leaves a zero mean at (0, 0, 0)).  ``normals``: [bs,N,3] fp64 on the device.

    Returns ``(points [bs,cap,3] fp32, normals [bs,cap,3] fp64, counts [bs] int32)``; rows beyond a cloud's count are zero.
    ``capacity=None`` reads the voxel counts on the host ONCE and sizes the outputs exactly (cap = the largest count).  An explicit
    ``capacity`` keeps the call free of host synchronisation and capturable in a graph; a cloud with more occupied voxels than
    ``capacity`` then comes back with count -1 and zero rows (CAPACITY_RULE)."""
    lib = _lib.load()
    v, cap, path = _radius(voxel_size, "voxel_size"), _capacity(capacity), _path(path)
    pts, n_dev = _cloud_batch(points, counts)
    bs, n = int(pts.shape[0]), int(pts.shape[1])
    if not torch.is_tensor(normals):
        raise TypeError("normals must be a tensor")
    normals = _chk(normals, "normals", torch.float64)
    if tuple(normals.shape) != (bs, n, 3) or normals.device != pts.device:
        raise ValueError(f"normals must be [{bs},{n},3] fp64 on {pts.device}, got {tuple(normals.shape)} on {normals.device}")
    return _voxel_with_normals(lib, pts, n_dev, normals, v, cap, renormalize, path)


@_on_device
def extract_fpfh_features(points: Points, voxel_size: float, counts: Optional[torch.Tensor] = None, viewpoint=None,
                          capacity: Optional[int] = None, renormalize: bool = False, path: str = "auto") -> Dict[str, torch.Tensor]:
    """``demo_registration.py:37-44`` (``extract_fpfh_features``) for a padded or ragged batch of RAW clouds: ``estimate_normals``
    with (2 voxel, 30) on the raw cloud (NORMAL_SIGN_RULE towards ``viewpoint``), ``voxel_down_sample(voxel_size)`` with averaged
    normals (``voxel_down_sample_with_normals``), ``compute_fpfh_feature`` with (5 voxel, 100) on the down-sampled cloud and those
    normals, then ``f / (|f|_2 + 1e-6)``.

    Returns ``points`` [bs,cap,3] fp32, ``desc`` [bs,cap,33] fp32, ``fpfh`` [bs,cap,33] fp64, ``normals`` [bs,cap,3] fp64 and
    ``counts`` [bs] int32 (all on the device; rows beyond a count are zero).  ``capacity=None`` reads the voxel counts on the host
    ONCE to size the outputs exactly; an explicit ``capacity`` makes the whole chain free of host synchronisation and capturable
    (CAPACITY_RULE: count -1 and zero rows for a cloud that does not fit)."""
    lib = _lib.load()
    v, cap, vp, path_name, path = _radius(voxel_size, "voxel_size"), _capacity(capacity), _viewpoint(viewpoint), path, _path(path)
    pts, n_dev = _cloud_batch(points, counts)
    bs, n = int(pts.shape[0]), int(pts.shape[1])
    idx, _, count = _lists(lib, pts, n_dev, NORMAL_RADIUS_VOXELS * v, NORMAL_MAX_NN, want_d2=False, path=path)
    raw_normals = torch.empty(bs, n, 3, dtype=torch.float64, device=pts.device)
    _lib.check(lib.pdsc_estimate_normals(_p(pts), _p(n_dev), _p(idx), _p(count), NORMAL_MAX_NN, vp, _p(raw_normals), bs, n, _stream()),
               "pdsc_estimate_normals")
    del idx, count
    down, down_n, down_counts = _voxel_with_normals(lib, pts, n_dev, raw_normals, v, cap, renormalize, path)
    feat = compute_fpfh_feature(down, FEATURE_RADIUS_VOXELS * v, FEATURE_MAX_NN, normals=down_n, counts=down_counts, path=path_name)
    return {"points": down, "desc": feat["desc"], "fpfh": feat["fpfh"], "normals": down_n, "counts": down_counts}


__all__: List[str] = ["hybrid_neighbours", "estimate_normals", "compute_fpfh_feature", "fpfh_descriptors",
                      "voxel_down_sample_with_normals", "extract_fpfh_features", "FPFH_DIM"]
