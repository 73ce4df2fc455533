"""Correspondence RANSAC on the device.

``ransac_correspondence`` stands in for open3d's ``registration_ransac_based_on_correspondence`` as the reference's callers use it:
``baseline_scripts/baseline_3DMatch.py:80-98`` (``--method RANSAC``: ransac_n 4, 1000 iterations, every correspondence) and
``evaluation/test_3DMatch.py:59-77`` / ``test_KITTI.py:59-77`` (``--solver RANSAC``: ransac_n 3, 5000 iterations, the correspondences
the model labelled as inliers).  The contract -- counter-based draws (DRAW_RULE), fp64 Umeyama hypotheses, fp64 scoring over every
candidate (SCORE_RULE), the selection order (SELECT_RULE), no refit (NO_REFIT_RULE) -- is written out in include/pointdsc_hip.h; it
does not reproduce open3d's random draws.  The arithmetic runs in libpointdsc_hip.so (``pdsc_ransac_correspondence``,
csrc/ransac.hip): four launches, no host synchronisation, so the call can sit inside the timed model window and inside a captured
graph.  GPU only.

Inputs are ``[bs,N,3]`` tensors (every pair has N correspondences) or lists of per-pair ``[n_b,3]`` / ``[1,n_b,3]`` tensors (a ragged
batch: padded to the longest pair, per-pair counts on the device), as in ``icp.icp_refine``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Union

import torch

from . import _lib
from .icp import _as_batch, _counts
from .ops import _chk, _on_device, _p, _stream

Points = Union[torch.Tensor, Sequence[torch.Tensor]]

CHUNK = 512                 # PDSC_RANSAC_CHUNK: entries of the candidate list per partial sum of sumsq (part of the contract)
RANSAC_N_RANGE = (3, 8)


def _as_mask(mask, bs: int, n: int, counts: List[int], dev) -> Optional[torch.Tensor]:
    """-> [bs,n] fp32 on `dev` (candidates are the entries > 0), padded with zeros for a list of per-pair rows."""
    if mask is None:
        return None
    if torch.is_tensor(mask):
        if mask.dim() == 1 and bs == 1:
            mask = mask[None]
        if tuple(mask.shape) != (bs, n):
            raise ValueError(f"mask must be [{bs},{n}], got {tuple(mask.shape)}")
        if not mask.is_cuda:
            raise RuntimeError("mask must live on the GPU (pointdsc_amd has no CPU path)")
        return mask.detach().to(torch.float32).contiguous()
    rows = list(mask)
    if len(rows) != bs:
        raise ValueError(f"mask has {len(rows)} rows, the batch {bs} pairs")
    out = torch.zeros(bs, n, device=dev, dtype=torch.float32)
    for i, r in enumerate(rows):
        r = r.reshape(-1)
        if not r.is_cuda:
            raise RuntimeError("mask must live on the GPU (pointdsc_amd has no CPU path)")
        if r.numel() != counts[i]:
            raise ValueError(f"mask[{i}] has {r.numel()} entries, the pair {counts[i]} correspondences")
        out[i, :counts[i]] = r.detach().to(torch.float32)
    return out


@_on_device
def ransac_correspondence(src_keypts: Points, tgt_keypts: Points, max_correspondence_distance: float = 0.10, ransac_n: int = 3,
                          max_iteration: int = 5000, max_validation: Optional[int] = None, mask=None, seed: int = 0,
                          pair_offset: int = 0, samples: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                          return_info: Union[bool, str] = False):
    """RANSAC over given correspondences for every pair of the batch: row i of ``src_keypts`` corresponds to row i of
    ``tgt_keypts``.  ``I = min(max_iteration, max_validation or max_iteration)`` hypotheses (baseline_3DMatch.py:90).
    ``mask`` ([bs,N], or a list of per-pair rows): the candidates are the correspondences with mask > 0 (None: all).
    ``seed`` (64-bit) and ``pair_offset`` (the index of the call's first pair in the caller's sequence) fix the draws: a pair's
    result does not depend on the batch it runs in.  ``samples`` [bs,I,ransac_n] int32 (positions into the candidate list) replaces the
    draws.  ``counts`` [bs] int32 on the device gives the valid rows of padded ``[bs,N,3]`` inputs without a host read.

    Returns ``(trans [bs,4,4] fp32, labels [bs,N] fp32)`` -- for list input ``labels`` is a list of per-pair [n_b] rows; identity and
    zeros where nothing won (fewer candidates than ransac_n, a threshold <= 0 or NaN, no hypothesis with an inlier).
    ``return_info=True`` adds a dict of device tensors: ``fitness``, ``inlier_rmse`` [bs] fp64, ``best_iter`` [bs] int32 (-1: nothing
    won), ``num_candidates`` [bs] int32; ``return_info="table"`` also the hypothesis table ``hyp_trans`` [bs,I,3,4] fp64 (NaN for an
    invalid hypothesis), ``hyp_count`` [bs,I] int32, ``hyp_sumsq`` [bs,I] fp64; ``return_info="stages"`` (tools/ransac_bench.py)
    adds ``stage_ms``, the event times of the four launches -- that call synchronises the host."""
    lib = _lib.load()
    n_s = int(ransac_n)
    if not RANSAC_N_RANGE[0] <= n_s <= RANSAC_N_RANGE[1]:
        raise ValueError(f"ransac_n must be in {RANSAC_N_RANGE[0]}..{RANSAC_N_RANGE[1]}, got {ransac_n}")
    I = min(int(max_iteration), int(max_validation) if max_validation else int(max_iteration))
    if I < 1:
        raise ValueError(f"max_iteration / max_validation must be >= 1, got {max_iteration} / {max_validation}")
    if return_info not in (False, True, "table", "stages"):
        raise ValueError(f"return_info must be False, True, 'table' or 'stages', got {return_info!r}")
    ragged = not torch.is_tensor(src_keypts)
    src, n_src, c_dev = _as_batch(src_keypts, "src_keypts")
    tgt, n_tgt, _ = _as_batch(tgt_keypts, "tgt_keypts")
    if n_src != n_tgt:
        raise ValueError("src_keypts and tgt_keypts must have the same number of rows per pair (row i is correspondence i)")
    if src.device != tgt.device:
        raise ValueError("src_keypts and tgt_keypts must live on the same device")
    bs, n, dev = int(src.shape[0]), int(src.shape[1]), src.device
    if counts is not None:
        if c_dev is not None:
            raise ValueError("counts goes with padded [bs,N,3] tensors, not with lists of pairs")
        c_dev = _counts(counts, bs, dev, "counts")
    m = _as_mask(mask, bs, n, n_src, dev)
    if samples is not None:
        if not torch.is_tensor(samples):
            raise TypeError("samples must be a tensor")
        samples = _chk(samples, "samples", torch.int32)
        if tuple(samples.shape) != (bs, I, n_s) or samples.device != dev:
            raise ValueError(f"samples must be [{bs},{I},{n_s}] int32 on {dev}, got {tuple(samples.shape)} on {samples.device}")
    ws_bytes = int(lib.pdsc_ransac_workspace_bytes(bs, n, I))
    if ws_bytes == 0:
        raise ValueError(f"unsupported sizes: bs={bs} N={n} max_iteration={I}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    trans = torch.empty(bs, 4, 4, dtype=torch.float32, device=dev)
    labels = torch.empty(bs, n, dtype=torch.float32, device=dev)
    fitness = torch.empty(bs, dtype=torch.float64, device=dev)
    rmse = torch.empty(bs, dtype=torch.float64, device=dev)
    best = torch.empty(bs, dtype=torch.int32, device=dev)
    ncand = torch.empty(bs, dtype=torch.int32, device=dev)
    table = return_info == "table"
    hyp_trans = torch.empty(bs, I, 3, 4, dtype=torch.float64, device=dev) if table else None
    hyp_count = torch.empty(bs, I, dtype=torch.int32, device=dev) if table else None
    hyp_sumsq = torch.empty(bs, I, dtype=torch.float64, device=dev) if table else None
    args = [_p(src), _p(tgt), _p(c_dev), _p(m), _p(samples), float(max_correspondence_distance), n_s, I,
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(pair_offset), _p(trans), _p(labels), _p(fitness), _p(rmse), _p(best), _p(ncand),
            _p(hyp_trans), _p(hyp_count), _p(hyp_sumsq), _p(ws), ws_bytes, bs, n]
    stage_ms = (C.c_float * 4)() if return_info == "stages" else None
    if stage_ms is not None:                                     # tools/ransac_bench.py: event times per launch; synchronises the host
        _lib.check(lib.pdsc_ransac_correspondence_stages(*args, stage_ms, _stream()), "pdsc_ransac_correspondence_stages")
    else:
        _lib.check(lib.pdsc_ransac_correspondence(*args, _stream()), "pdsc_ransac_correspondence")
    out_labels = [labels[i, :k] for i, k in enumerate(n_src)] if ragged else labels
    if not return_info:
        return trans, out_labels
    info = {"fitness": fitness, "inlier_rmse": rmse, "best_iter": best, "num_candidates": ncand, "max_iteration": I}
    if stage_ms is not None:
        info["stage_ms"] = list(stage_ms)                        # compact | hypothesise | score | select
    if table:
        info.update(hyp_trans=hyp_trans, hyp_count=hyp_count, hyp_sumsq=hyp_sumsq)
    return trans, out_labels, info


__all__: List[str] = ["ransac_correspondence", "CHUNK"]
