"""Classical baselines of the reference that share the hot path's kernels.

``SM`` mirrors ``baseline_scripts/baseline_3DMatch.py:19-53`` (spectral matching: N x N compatibility matrix + 10 power
iterations + top-10 % selection + weighted Procrustes) with the reference's argument meaning; the arithmetic runs in
``csrc/spectral.hip`` (matrix written once, one HBM-bound mat-vec launch per iteration).  ``PMC`` (:56-77) is the exact maximum
clique of ``csrc/pmc.hip``; ``RANSAC`` (:80-98) is correspondence RANSAC under the project's own contract (``ransac.py``,
``csrc/ransac.hip``).  GPU only.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def SM(corr: torch.Tensor, src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, inlier_threshold: float, top_ratio: float = 0.1,
       num_iterations: int = 10, return_eig: bool = False, form: str = "auto"):
    """corr [N,6] (or [bs,N,6]) centred correspondence coordinates, src/tgt_keypts [bs,N,3] ->
    (pred_trans [bs,4,4], pred_labels [bs,N]) like the reference's SM(corr, src_keypts, tgt_keypts, args, top_ratio)
    with ``args.inlier_threshold`` passed explicitly; bs > 1 = independent pairs.  A NaN distance difference (a NaN or
    inf coordinate) makes that pair's eigenvector and pose NaN, as in the reference.
    ``form``: "streaming" (matrix in HBM, N <= 40 896),
    "resident" (opt-in: the matrix stays in the chip's vector registers, N <= 5120; needs the GPU to itself -- cooperative launch,
    refused under graph capture) or "auto" (= "streaming", always); same bits either way."""
    forms = {"auto": 0, "streaming": 1, "resident": 2}
    if form not in forms:
        raise ValueError(f"form must be one of {sorted(forms)}, got {form!r}")
    lib = _lib.load()
    if not corr.is_cuda:
        raise RuntimeError("pointdsc_amd has no CPU path: move the tensors to the GPU")
    src = src_keypts.detach().to(torch.float32).contiguous()
    tgt = tgt_keypts.detach().to(torch.float32).contiguous()
    bs, n = src.shape[0], src.shape[1]
    c = corr.detach().to(torch.float32).reshape(bs, n, 6).contiguous()
    dev = c.device
    num_top = int(n * top_ratio)                               # python double arithmetic, as the reference (:47)
    trans = torch.empty(bs, 4, 4, device=dev, dtype=torch.float32)
    labels = torch.empty(bs, n, device=dev, dtype=torch.float32)
    eig = torch.empty(bs, n, device=dev, dtype=torch.float32)
    nb = int(lib.pdsc_sm_workspace_bytes(bs, n))
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        rc = lib.pdsc_sm_baseline_form(C.c_void_p(c.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(tgt.data_ptr()),
                                       float(inlier_threshold), num_top, int(num_iterations), C.c_void_p(trans.data_ptr()),
                                       C.c_void_p(labels.data_ptr()), C.c_void_p(eig.data_ptr()), C.c_void_p(ws.data_ptr()), nb,
                                       bs, n, forms[form], torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "pdsc_sm_baseline")
    return (trans, labels, eig) if return_eig else (trans, labels)


CONFIDENCE_METHODS = {"eig_value": 0, "eig_value_ratio": 1, "xMx": 2}


def cal_confidence(M: torch.Tensor, leading_eig: torch.Tensor, method: str = "eig_value", num_iterations: int = 10) -> torch.Tensor:
    """``PointDSC.cal_confidence`` (reference models/PointDSC.py:366-401): M [bs,N,N] (or [bs,N,ld], ld >= N a multiple of 4,
    e.g. the matrix of ``ops.spatial_compat``), leading_eig [bs,N] -> confidence [bs,1] with the reference's three
    methods; ``num_iterations`` = the module's power-iteration count (used by 'eig_value_ratio')."""
    lib = _lib.load()
    if method not in CONFIDENCE_METHODS:
        raise ValueError(f"method must be one of {sorted(CONFIDENCE_METHODS)}")
    if not M.is_cuda:
        raise RuntimeError("pointdsc_amd has no CPU path: move the tensors to the GPU")
    v = leading_eig.detach().to(torch.float32).contiguous()
    bs, n = v.shape
    m = M.detach().to(torch.float32)
    if m.shape[-1] % 4 != 0:                                 # float4 row loads
        m = torch.nn.functional.pad(m, (0, 4 - m.shape[-1] % 4))
    m = m.contiguous()
    ld = m.shape[-1]
    conf = torch.empty(bs, device=m.device, dtype=torch.float32)
    nb = int(lib.pdsc_cal_confidence_workspace_bytes(bs, n))
    ws = torch.empty(nb, device=m.device, dtype=torch.uint8)
    with torch.cuda.device(m.device):
        rc = lib.pdsc_cal_confidence(C.c_void_p(m.data_ptr()), ld, C.c_void_p(v.data_ptr()), CONFIDENCE_METHODS[method],
                                     int(num_iterations), C.c_void_p(conf.data_ptr()), C.c_void_p(ws.data_ptr()), nb, bs, n,
                                     torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "pdsc_cal_confidence")
    return conf[:, None]


# branching steps per workgroup and launch: the hard instance of tools/pmc_bench.py (500 inliers, ~90 % dense) is proven in 0.25 s,
# a pair of N = 5000 with 500 inliers returns unproven in 0.8 s (DESIGN.md section 8 f-10 has the measurements)
PMC_DEFAULT_MAX_NODES = 10000


def pmc_adjacency(corr: torch.Tensor, inlier_threshold: float, ld_words: int = 0) -> torch.Tensor:
    """Edge bitset of the PMC compatibility graph: corr [bs,N,6] -> int64 [bs,N,ld_words] (ld_words >= ceil(N/64), default that),
    bit (j & 63) of word (j >> 6) of row i = |sum((c_i[0:3]-c_j[0:3])**2) - sum((c_i[3:6]-c_j[3:6])**2)| < inlier_threshold, the
    fp32 arithmetic of baseline_3DMatch.py:66-67 bit for bit; zero diagonal, padding bits zero."""
    lib = _lib.load()
    if not corr.is_cuda:
        raise RuntimeError("pointdsc_amd has no CPU path: move the tensors to the GPU")
    c = corr.detach().to(torch.float32).contiguous()
    bs, n = c.shape[0], c.shape[1]
    ld = int(ld_words) if ld_words else max(1, (n + 63) // 64)
    bits = torch.empty(bs, n, ld, device=c.device, dtype=torch.int64)
    with torch.cuda.device(c.device):
        rc = lib.pdsc_pmc_adjacency(C.c_void_p(c.data_ptr()), float(inlier_threshold), C.c_void_p(bits.data_ptr()), ld, bs, n,
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "pdsc_pmc_adjacency")
    return bits


def pmc_run(corr: torch.Tensor, src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, inlier_threshold: float,
            max_nodes: int = PMC_DEFAULT_MAX_NODES, stages: bool = False, lds_words: int = 0) -> dict:
    """One pdsc_pmc_baseline call with everything it leaves behind: pred_trans, pred_labels, clique_size, proven and ``counters``
    [bs,4] int64 (nodes expanded, roots that branched, roots not exhausted, the greedy bound -- read from the workspace head).
    ``stages`` (tools/pmc_bench.py) adds ``stage_ms`` = milliseconds of adjacency | ordering and bound | search | labels and
    Procrustes; that call synchronises the host.  ``lds_words`` (tests) restricts the LDS pool of the first search pass, so that roots
    take the slab pass (pdsc_pmc_baseline_ex)."""
    lib = _lib.load()
    if not corr.is_cuda:
        raise RuntimeError("pointdsc_amd has no CPU path: move the tensors to the GPU")
    src = src_keypts.detach().to(torch.float32).contiguous()
    tgt = tgt_keypts.detach().to(torch.float32).contiguous()
    bs, n = src.shape[0], src.shape[1]
    c = corr.detach().to(torch.float32).reshape(bs, n, 6).contiguous()
    dev = c.device
    trans = torch.empty(bs, 4, 4, device=dev, dtype=torch.float32)
    labels = torch.empty(bs, n, device=dev, dtype=torch.float32)
    size = torch.empty(bs, device=dev, dtype=torch.int32)
    proven = torch.empty(bs, device=dev, dtype=torch.int32)
    nb = int(lib.pdsc_pmc_workspace_bytes(bs, n))
    ws = torch.empty(max(nb, 32 * bs), device=dev, dtype=torch.uint8)
    args = [C.c_void_p(c.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(tgt.data_ptr()), float(inlier_threshold), int(max_nodes),
            C.c_void_p(trans.data_ptr()), C.c_void_p(labels.data_ptr()), C.c_void_p(size.data_ptr()), C.c_void_p(proven.data_ptr()),
            C.c_void_p(ws.data_ptr()), nb, bs, n]
    out = {"pred_trans": trans, "pred_labels": labels, "clique_size": size, "proven": proven}
    with torch.cuda.device(dev):
        if stages or lds_words:
            ms = (C.c_float * 4)() if stages else None
            rc = lib.pdsc_pmc_baseline_ex(*args, int(lds_words), ms, torch.cuda.current_stream().cuda_stream)
            if stages:
                out["stage_ms"] = list(ms)
        else:
            rc = lib.pdsc_pmc_baseline(*args, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "pdsc_pmc_baseline")
    out["counters"] = ws[:32 * bs].view(torch.int64).reshape(bs, 4)
    return out


def PMC(corr: torch.Tensor, src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, inlier_threshold: float,
        max_nodes: int = PMC_DEFAULT_MAX_NODES, return_info: bool = False):
    """The reference's PMC(corr, src_keypts, tgt_keypts, args) (baseline_3DMatch.py:56-77) with ``args.inlier_threshold`` passed
    explicitly: corr [N,6] (or [bs,N,6]), src/tgt_keypts [bs,N,3] -> (pred_trans [bs,4,4], pred_labels [bs,N]); pred_labels is 1 on
    a maximum clique of the compatibility graph (edge rule: ``pmc_adjacency``), pred_trans = rigid_transform_3d(src, tgt, pred_labels).
    bs > 1 = independent pairs.  ``max_nodes`` bounds the branch and bound: branching steps per workgroup and launch, a workgroup being
    one root's search (include/pointdsc_hip.h has the rule for roots too large for LDS);
    when a root runs out the best clique found is returned and ``proven`` is 0.  ``return_info`` adds (clique_size [bs] int32,
    proven [bs] int32).  A graph without edges labels vertex 0 alone (the reference raises there); the result is deterministic
    (tie rule: include/pointdsc_hip.h).  GPU only."""
    r = pmc_run(corr, src_keypts, tgt_keypts, inlier_threshold, max_nodes)
    if return_info:
        return r["pred_trans"], r["pred_labels"], r["clique_size"], r["proven"]
    return r["pred_trans"], r["pred_labels"]


def RANSAC(corr, src_keypts, tgt_keypts, inlier_threshold: float, max_iteration: int = 1000, max_validation: int = 1000, seed: int = 0,
           pair_offset: int = 0):
    """The reference's RANSAC(corr, src_keypts, tgt_keypts, args) (baseline_3DMatch.py:80-98: open3d
    registration_ransac_based_on_correspondence over all N correspondences, ransac_n = 4, RANSACConvergenceCriteria(max_iteration,
    max_validation)) with ``args.inlier_threshold`` passed explicitly: src/tgt_keypts [bs,N,3] (or lists of per-pair [N,3] tensors)
    -> (pred_trans [bs,4,4], pred_labels [bs,N]); ``corr`` is accepted and unused, as in the reference.  The hypotheses number
    min(max_iteration, max_validation) (:90); ``seed`` and ``pair_offset`` fix the draws (``ransac.ransac_correspondence`` has the
    contract: it does not reproduce open3d's random draws).  GPU only."""
    from .ransac import ransac_correspondence
    return ransac_correspondence(src_keypts, tgt_keypts, inlier_threshold, ransac_n=4, max_iteration=max_iteration,
                                 max_validation=max_validation, seed=seed, pair_offset=pair_offset)
