"""Correspondence construction on the GPU -- the step in front of ``PointDSC.forward``.

Mirrors what the reference does with numpy on the host inside its datasets / demo:

    datasets/ThreeDMatch.py:283-290   distance = sqrt(2 - 2 * src_desc @ tgt_desc.T + 1e-6); argmin (+ mutual check)
    datasets/ThreeDMatch.py:299-308   gather the keypoints, corr_pos = concat(src, tgt) - mean       (in_dim = 6)
    demo_registration.py:101-108      the same without the mutual check
    evaluation/test_3DLoMatch.py:45-48  the torch form of the 3DLoMatch caller: argmax of the inner products (metric="ip");
                                        equal to the arg-min above only for exactly unit-length descriptors

``build_correspondences`` returns exactly the three tensors the forward consumes (plus the index pairs), batched as
``[1, Nc, .]`` like the reference's data loader hands them over.  The Ns x Nt distance matrix is never materialised:
one fused MFMA GEMM + arg-min kernel (csrc/match.hip).  GPU only; no CPU fallback.

``build_correspondences_batch`` does the same for a batch of pairs over a pool of clouds in one library call, with the data
loader's ground-truth label (datasets/ThreeDMatch.py:293-297, fp64) when asked for (csrc/match_batch.hip).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    return t.detach().to(torch.float32).contiguous()


def match_descriptors(src_desc: torch.Tensor, tgt_desc: torch.Tensor, want_dist: bool = False, metric: str = "l2"):
    """nn_idx [Ns] int32 (and nn_dist [Ns]) of ``argmin(sqrt(2 - 2 * src_desc @ tgt_desc.T + 1e-6), axis=1)`` (metric "l2"), or of
    ``argmax(src_desc @ tgt_desc.T, dim=-1)`` (metric "ip", evaluation/test_3DLoMatch.py:45-46; nn_dist is then the inner product)."""
    if metric not in ("l2", "ip"):
        raise ValueError(f'metric must be "l2" or "ip", got {metric!r}')
    lib = _lib.load()
    s, t = _chk(src_desc, "src_desc"), _chk(tgt_desc, "tgt_desc")
    ns, d = s.shape
    nt = t.shape[0]
    if t.shape[1] != d:
        raise ValueError("descriptor lengths differ")
    idx = torch.empty(ns, device=s.device, dtype=torch.int32)
    dist = torch.empty(ns, device=s.device, dtype=torch.float32) if want_dist else None
    nb = int(lib.pdsc_match_scratch_bytes(ns, nt))
    scratch = torch.empty(nb, device=s.device, dtype=torch.uint8)
    with torch.cuda.device(s.device):
        fn = lib.pdsc_match_descriptors if metric == "l2" else lib.pdsc_match_descriptors_ip
        _lib.check(fn(_p(s), _p(t), ns, nt, d, _p(idx), _p(dist), _p(scratch), nb, torch.cuda.current_stream().cuda_stream),
                   "pdsc_match_descriptors" + ("" if metric == "l2" else "_ip"))
    return (idx, dist) if want_dist else idx


def build_correspondences(src_desc: torch.Tensor, tgt_desc: torch.Tensor, src_keypts: torch.Tensor,
                          tgt_keypts: torch.Tensor, use_mutual: bool = False, metric: str = "l2") -> Dict[str, torch.Tensor]:
    """descriptors [Ns,D] / [Nt,D] (L2-normalised), keypoints [Ns,3] / [Nt,3]  ->
    {'corr_pos' [1,Nc,6], 'src_keypts' [1,Nc,3], 'tgt_keypts' [1,Nc,3], 'corr' [Nc,2] int32}.
    ``use_mutual`` keeps only mutual nearest neighbours (ThreeDMatch.py:286-288); Nc is then data dependent, which costs
    the one host synchronisation that reads it.  ``metric="ip"`` matches by the largest inner product, as the 3DLoMatch caller
    does (evaluation/test_3DLoMatch.py:45-48)."""
    lib = _lib.load()
    skp, tkp = _chk(src_keypts, "src_keypts"), _chk(tgt_keypts, "tgt_keypts")
    s2t = match_descriptors(src_desc, tgt_desc, metric=metric)
    t2s = match_descriptors(tgt_desc, src_desc, metric=metric) if use_mutual else None
    ns, dev = s2t.shape[0], s2t.device
    corr = torch.empty(ns, 2, device=dev, dtype=torch.int32)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    corr_pos = torch.empty(ns, 6, device=dev, dtype=torch.float32)
    src_sel = torch.empty(ns, 3, device=dev, dtype=torch.float32)
    tgt_sel = torch.empty(ns, 3, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.pdsc_select_correspondences(_p(s2t), _p(t2s), ns, _p(corr), _p(count), st), "pdsc_select_correspondences")
        _lib.check(lib.pdsc_build_corr_pos(_p(skp), _p(tkp), _p(corr), _p(count), _p(corr_pos), _p(src_sel), _p(tgt_sel), st),
                   "pdsc_build_corr_pos")
    nc = int(count.item()) if use_mutual else ns
    return {"corr_pos": corr_pos[None, :nc], "src_keypts": src_sel[None, :nc], "tgt_keypts": tgt_sel[None, :nc],
            "corr": corr[:nc]}


# -------------------------------------------------------------------------------------------------------------------------
# a batch of pairs over a pool of clouds (csrc/match_batch.hip)
# -------------------------------------------------------------------------------------------------------------------------
MATCH_TILE = 128                    # MT_SRC of csrc/match_tile.h: source rows per matcher workgroup
MATCH_MAX_D = 64                    # MT_MAXD


class CorrPool:
    """The clouds of a pool, concatenated once: ``desc`` [total, D] and ``keypts`` [total, 3] fp32 on the device, ``counts`` and
    ``offsets`` (host lists, from the shapes).  ``build_correspondences_batch`` takes one in place of its ``desc`` list, so that a
    driver that batches many groups of pairs over the same clouds concatenates them once."""

    def __init__(self, desc: Sequence[torch.Tensor], keypts: Sequence[torch.Tensor]):
        desc, keypts = list(desc), list(keypts)
        if not desc or len(desc) != len(keypts):
            raise ValueError("desc and keypts must be lists of the same (non-zero) length: one entry per cloud of the pool")
        d = int(desc[0].shape[-1]) if desc[0].dim() == 2 else -1
        for v, (a, k) in enumerate(zip(desc, keypts)):
            if a.dim() != 2 or k.dim() != 2 or int(a.shape[1]) != d or int(k.shape[1]) != 3 or a.shape[0] != k.shape[0] or a.shape[0] < 1:
                raise ValueError(f"cloud {v}: desc must be [n, {d}] and keypts [n, 3] with the same n >= 1, "
                                 f"got {tuple(a.shape)} and {tuple(k.shape)}")
        if not 1 <= d <= MATCH_MAX_D:
            raise ValueError(f"descriptor length {d}: the matcher holds 1 .. {MATCH_MAX_D} columns")
        self.counts = [int(a.shape[0]) for a in desc]
        self.offsets = [0]
        for n in self.counts[:-1]:
            self.offsets.append(self.offsets[-1] + n)
        self.dim = d
        self.desc = torch.cat([_chk(a, "desc") for a in desc])
        self.keypts = torch.cat([_chk(k, "keypts") for k in keypts]).to(self.desc.device)
        self.device = self.desc.device


def _pair_list(pairs, num_clouds: int) -> List[Tuple[int, int]]:
    """`pairs` as a host list of (source, target); a tensor is read where it lives (a device tensor costs a read: pass host indices)."""
    rows = pairs.tolist() if torch.is_tensor(pairs) else [tuple(p) for p in pairs]
    if not rows or any(len(r) != 2 for r in rows):
        raise ValueError("pairs must be a non-empty [P, 2] list of (source, target) pool indices")
    out = []
    for s, t in rows:
        if int(s) != s or int(t) != t or not (0 <= s < num_clouds and 0 <= t < num_clouds):
            raise ValueError(f"pair ({s}, {t}) is outside the pool of {num_clouds} clouds")
        out.append((int(s), int(t)))
    return out


def build_correspondences_batch(desc, keypts, pairs, use_mutual: bool = False, metric: str = "l2", gt_trans=None,
                                inlier_threshold: Optional[float] = None, _splits: int = 0) -> Dict[str, object]:
    """``build_correspondences`` for P pairs of a pool of clouds in ONE library call (five launches, no host read).

    ``desc`` / ``keypts``: lists of per-cloud [n_v, D] / [n_v, 3] GPU tensors (or a ``CorrPool`` and None); ``pairs``: sequence or
    int tensor [P, 2] of (source, target) pool indices -- repeats, both orders of a pair and s == t are allowed.
    Returns, padded to ``cap`` = the largest source count of the batch with ZERO rows behind each pair's count:
    ``corr_pos`` [P,cap,6], ``src_keypts`` / ``tgt_keypts`` [P,cap,3], ``corr`` [P,cap,2] int32, ``num_corr`` [P] int32 on the device,
    ``num_corr_host`` (the counts as a list, known from the shapes, when ``use_mutual`` is False; else None: reading ``num_corr`` is
    the caller's choice) and, with ``gt_trans`` ([P,4,4], taken to fp64) and ``inlier_threshold``, ``gt_labels`` [P,cap] fp32:
    ``sqrt(sum((R src + t - tgt)^2)) < inlier_threshold`` in fp64 (datasets/ThreeDMatch.py:293-297).
    Pair p's rows are bit for bit those of ``build_correspondences`` on that pair.  With ``testing`` added and ``num_corr`` set to
    ``num_corr_host`` (or left as the device tensor) the dictionary is an input of ``PointDSC.forward``; pairs with fewer than two
    correspondences are the caller's to drop.  Never synchronises."""
    if metric not in ("l2", "ip"):
        raise ValueError(f'metric must be "l2" or "ip", got {metric!r}')
    if (gt_trans is None) != (inlier_threshold is None):
        raise ValueError("gt_trans and inlier_threshold go together (both, or neither)")
    plist = _pair_list(pairs, len(desc.counts) if isinstance(desc, CorrPool) else len(desc))
    pool = desc if isinstance(desc, CorrPool) else CorrPool(desc, keypts)
    P, dev = len(plist), pool.device
    items = [w for s, t in plist for w in ((s, t), (t, s))] if use_mutual else plist
    table, tile = [], 0
    for s, t in items:
        table.append((pool.offsets[s], pool.counts[s], pool.offsets[t], pool.counts[t], tile))
        tile += -(-pool.counts[s] // MATCH_TILE)
    cap = max(pool.counts[s] for s, _ in plist)
    max_tgt = max(pool.counts[t] for _, t in items)
    gt = None
    if gt_trans is not None:
        thr = float(inlier_threshold)
        if thr != thr:
            raise ValueError("inlier_threshold is NaN")
        gt = (gt_trans if torch.is_tensor(gt_trans) else torch.as_tensor(gt_trans)).detach()
        if tuple(gt.shape) != (P, 4, 4) or not gt.is_floating_point():
            raise ValueError(f"gt_trans must be a float [{P}, 4, 4] tensor, got {tuple(gt.shape)} {gt.dtype}")
        gt = gt.to(device=dev, dtype=torch.float64, non_blocking=True).contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        table_dev = torch.tensor(table, dtype=torch.int32).to(dev, non_blocking=True)       # the one upload: shapes only
        f32 = dict(device=dev, dtype=torch.float32)
        corr_pos, src_sel, tgt_sel = torch.empty(P, cap, 6, **f32), torch.empty(P, cap, 3, **f32), torch.empty(P, cap, 3, **f32)
        corr = torch.empty(P, cap, 2, device=dev, dtype=torch.int32)
        num_corr = torch.empty(P, device=dev, dtype=torch.int32)
        labels = torch.empty(P, cap, **f32) if gt is not None else None
        nb = int(lib.pdsc_corr_batch_workspace_bytes(P, tile, cap))
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        _lib.check(lib.pdsc_build_correspondences_batch_ex(
            _p(pool.desc), _p(pool.keypts), _p(table_dev), P, pool.dim, int(bool(use_mutual)), 0 if metric == "l2" else 1, tile, max_tgt,
            cap, _p(gt), float(inlier_threshold) if gt is not None else 0.0, _p(corr_pos), _p(src_sel), _p(tgt_sel), _p(corr),
            _p(num_corr), _p(labels), _p(ws), nb, int(_splits), torch.cuda.current_stream().cuda_stream),
            "pdsc_build_correspondences_batch")
    out = {"corr_pos": corr_pos, "src_keypts": src_sel, "tgt_keypts": tgt_sel, "corr": corr, "num_corr": num_corr,
           "num_corr_host": None if use_mutual else [pool.counts[s] for s, _ in plist]}
    if labels is not None:
        out["gt_labels"] = labels
    return out
