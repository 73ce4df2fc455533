"""The losses of the reference's ``libs/loss.py`` on the device, with their gradients (include/pointdsc_hip.h, section f-11).

``ClassificationLoss``, ``SpectralMatchingLoss`` and ``TransformationLoss`` keep the reference's constructor arguments, call
signatures and return shapes, so ``Trainer.evaluate_metric`` (libs/trainer.py:186-194) can hold them unchanged.  All arithmetic
runs in libpointdsc_hip.so: fp64 sums of fp64 per-element terms, deterministic (no atomics).  The loss values are fp32 0-dim device
tensors (the rounding of the library's fp64 slot); the classification loss, both forms of the spectral-matching loss and (f-14) the
transformation loss are ``torch.autograd.Function``s whose backward scales the gradient the kernels computed for an upstream gradient of 1 -- the
gradient buffers are requested only when an input requires a gradient.  There is no CPU path.

The ``*_raw`` functions are the thin wrappers over the C entry points (fp64 slots, fp64 / fp32 gradient buffers as the library
writes them); the modules are built on them.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from .ops import _chk, _on_device, _p, _stream

def _workspace(bs: int, n: int, dev) -> torch.Tensor:
    nbytes = int(_lib.load().pdsc_loss_workspace_bytes(bs, n))
    if nbytes == 0:
        raise ValueError(f"unsupported loss problem size bs={bs} N={n}")
    return torch.empty(nbytes // 8, device=dev, dtype=torch.float64)


def _labels(gt: torch.Tensor, name: str = "gt") -> torch.Tensor:
    return _chk(gt.detach().to(torch.float32), name)


def _need_gpu(*named) -> None:
    """Before anything touches the library: a CPU tensor is this package's usual error, whether or not the library is built."""
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")


# ---------------------------------------------------------------------------------------------------------------------------
# raw wrappers
# ---------------------------------------------------------------------------------------------------------------------------
CLASSIFICATION_STATS = ("loss", "precision", "recall", "f1", "logit_true", "logit_false", "num_pos", "num_neg")
TRANSFORMATION_STATS = ("loss", "recall", "RE", "TE", "RMSE")


@_on_device
def classification_loss_raw(pred: torch.Tensor, gt: torch.Tensor, weight: Optional[torch.Tensor] = None, balanced: bool = True,
                            want_grad: bool = False):
    """pred, gt [bs,N] (+ weight [bs,N]) -> (stats fp64 [8] = CLASSIFICATION_STATS, dpred fp64 [bs,N] or None)."""
    _need_gpu(("pred", pred), ("gt", gt), ("weight", weight))
    lib = _lib.load()
    pred, gt = _chk(pred.detach(), "pred"), _labels(gt)
    if pred.dim() != 2 or gt.shape != pred.shape:
        raise ValueError("pred and gt must be [bs, num_corr]")
    w = None if weight is None else _chk(weight.detach().to(torch.float32).expand_as(pred), "weight")
    bs, n = pred.shape
    ws = _workspace(bs, n, pred.device)
    stats = torch.empty(8, device=pred.device, dtype=torch.float64)
    dpred = torch.empty(bs, n, device=pred.device, dtype=torch.float64) if want_grad else None
    _lib.check(lib.pdsc_classification_loss(_p(pred), _p(gt), _p(w), int(bool(balanced)), _p(stats), _p(dpred), _p(ws),
                                            ws.numel() * 8, bs, n, _stream()), "pdsc_classification_loss")
    return stats, dpred


@_on_device
def sm_loss_matrix_raw(M: torch.Tensor, gt: torch.Tensor, balanced: bool = True, want_grad: bool = False):
    """M [bs,N,N], gt [bs,N] -> (loss fp64 [1], dM fp64 [bs,N,N] or None, per-pair values fp64 [bs])."""
    _need_gpu(("M", M), ("gt_labels", gt))
    lib = _lib.load()
    M, gt = _chk(M.detach(), "M"), _labels(gt, "gt_labels")
    bs, n = gt.shape
    if M.shape != (bs, n, n):
        raise ValueError("M must be [bs, num_corr, num_corr] and gt_labels [bs, num_corr]")
    ws = _workspace(bs, n, M.device)
    loss = torch.empty(1, device=M.device, dtype=torch.float64)
    dM = torch.empty(bs, n, n, device=M.device, dtype=torch.float64) if want_grad else None
    _lib.check(lib.pdsc_sm_loss_matrix(_p(M), n, _p(gt), int(bool(balanced)), _p(loss), _p(dM), _p(ws), ws.numel() * 8, bs, n,
                                       _stream()), "pdsc_sm_loss_matrix")
    return loss, dM, ws[:bs]


@_on_device
def sm_loss_features_raw(normed: torch.Tensor, sigma: torch.Tensor, gt: torch.Tensor, balanced: bool = True,
                         want_dnormed: bool = False, want_dsigma: bool = False):
    """normed [bs*N,128] (or [bs,N,128]), sigma [1], gt [bs,N] -> (loss fp64 [1], dnormed fp32 like normed or None, dsigma fp64 [1]
    or None, per-pair values fp64 [bs]): the loss of M = clamp(1 - (1 - F F^T) / sigma^2, 0, 1), M never stored."""
    _need_gpu(("normed", normed), ("sigma", sigma), ("gt_labels", gt))
    lib = _lib.load()
    normed, sig, gt = _chk(normed.detach(), "normed"), _chk(sigma.detach().reshape(-1), "sigma"), _labels(gt, "gt_labels")
    bs, n = gt.shape
    if normed.numel() != bs * n * 128 or normed.shape[-1] != 128 or sig.numel() != 1:
        raise ValueError("normed must hold bs * num_corr rows of 128 channels and sigma one value")
    ws = _workspace(bs, n, normed.device)
    loss = torch.empty(1, device=normed.device, dtype=torch.float64)
    dnormed = torch.empty(normed.shape, device=normed.device, dtype=torch.float32) if want_dnormed else None
    dsigma = torch.empty(1, device=normed.device, dtype=torch.float64) if want_dsigma else None
    _lib.check(lib.pdsc_sm_loss_features(_p(normed), _p(sig), _p(gt), int(bool(balanced)), _p(loss), _p(dnormed), _p(dsigma), _p(ws),
                                         ws.numel() * 8, bs, n, _stream()), "pdsc_sm_loss_features")
    return loss, dnormed, dsigma, ws[:bs]


@_on_device
def transformation_loss_raw(trans, gt_trans, src_keypts, tgt_keypts, probs, re_thre: float = 15.0, te_thre: float = 30.0):
    """-> fp64 [5] = TRANSFORMATION_STATS (loss, recall %, RE deg, TE cm, RMSE; means over the pairs, the reference's broadcast of
    the target over the batch included)."""
    _need_gpu(("trans", trans), ("gt_trans", gt_trans), ("src_keypts", src_keypts), ("tgt_keypts", tgt_keypts), ("probs", probs))
    lib = _lib.load()
    T, G = _chk(trans.detach(), "trans"), _chk(gt_trans.detach().to(torch.float32), "gt_trans")
    s, t, p = _chk(src_keypts.detach(), "src_keypts"), _chk(tgt_keypts.detach(), "tgt_keypts"), _chk(probs.detach(), "probs")
    bs, n = p.shape
    if T.shape != (bs, 4, 4) or G.shape != (bs, 4, 4) or s.shape != (bs, n, 3) or t.shape != (bs, n, 3):
        raise ValueError("bad shapes for the transformation loss")
    ws = _workspace(bs, n, p.device)
    out = torch.empty(5, device=p.device, dtype=torch.float64)
    _lib.check(lib.pdsc_transformation_loss(_p(T), _p(G), _p(s), _p(t), _p(p), float(re_thre), float(te_thre), _p(out), _p(ws),
                                            ws.numel() * 8, bs, n, _stream()), "pdsc_transformation_loss")
    return out


@_on_device
def transformation_loss_grad_raw(trans, src_keypts, tgt_keypts, probs):
    """-> fp64 [bs,4,4] = d loss / d trans of transformation_loss_raw's loss (row 3 zero; the broadcast over the batch and the
    `some probs > 0` rule of the reference included).  pdsc_transformation_loss_grad."""
    _need_gpu(("trans", trans), ("src_keypts", src_keypts), ("tgt_keypts", tgt_keypts), ("probs", probs))
    lib = _lib.load()
    T = _chk(trans.detach(), "trans")
    s, t, p = _chk(src_keypts.detach(), "src_keypts"), _chk(tgt_keypts.detach(), "tgt_keypts"), _chk(probs.detach(), "probs")
    bs, n = p.shape
    if T.shape != (bs, 4, 4) or s.shape != (bs, n, 3) or t.shape != (bs, n, 3):
        raise ValueError("bad shapes for the transformation loss")
    ws = _workspace(bs, n, p.device)
    out = torch.empty(bs, 4, 4, device=p.device, dtype=torch.float64)
    _lib.check(lib.pdsc_transformation_loss_grad(_p(T), _p(s), _p(t), _p(p), _p(out), _p(ws), ws.numel() * 8, bs, n, _stream()),
               "pdsc_transformation_loss_grad")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------------------
def _wants_grad(t) -> bool:
    """Decided by the caller of Function.apply: inside Function.forward the grad mode is always off."""
    return torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled()


class _ClassificationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, weight, balanced, want):
        stats, dpred = classification_loss_raw(pred, gt, weight, balanced, want_grad=want)
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(stats)
        return stats[0].to(torch.float32), stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        (dpred,) = ctx.saved_tensors
        return (dpred * g_loss).to(torch.float32), None, None, None, None


class _SmMatrixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, gt, balanced, want):
        loss, dM, _ = sm_loss_matrix_raw(M, gt, balanced, want_grad=want)
        ctx.save_for_backward(dM)
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g_loss):
        (dM,) = ctx.saved_tensors
        return (dM * g_loss).to(torch.float32), None, None, None


class _SmFeaturesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normed, sigma, gt, balanced, want_dnormed, want_dsigma):
        loss, dnormed, dsigma, _ = sm_loss_features_raw(normed, sigma, gt, balanced, want_dnormed=want_dnormed,
                                                        want_dsigma=want_dsigma)
        ctx.save_for_backward(dnormed, dsigma)
        ctx.shapes = (normed.shape, sigma.shape)
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g_loss):
        dnormed, dsigma = ctx.saved_tensors
        gn = None if dnormed is None else (dnormed * g_loss).reshape(ctx.shapes[0])
        gs = None if dsigma is None else (dsigma * g_loss).to(torch.float32).reshape(ctx.shapes[1])
        return gn, gs, None, None, None, None


class _TransformationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trans, gt_trans, src_keypts, tgt_keypts, probs, re_thre, te_thre):
        out = transformation_loss_raw(trans, gt_trans, src_keypts, tgt_keypts, probs, re_thre, te_thre)
        ctx.save_for_backward(transformation_loss_grad_raw(trans, src_keypts, tgt_keypts, probs))
        ctx.mark_non_differentiable(out)
        return out[0].to(torch.float32), out

    @staticmethod
    def backward(ctx, g_loss, _g_out):
        (dtrans,) = ctx.saved_tensors
        return (dtrans * g_loss).to(torch.float32), None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's modules
# ---------------------------------------------------------------------------------------------------------------------------
class ClassificationLoss(nn.Module):
    """libs/loss.py:66-112.  forward(pred, gt, weight=None) -> {"loss": fp32 0-dim device tensor (differentiable in pred),
    "precision", "recall", "f1", "logit_true", "logit_false": Python floats (ONE copy of the 8-double stats row)}.
    device_stats=True: the five metrics are fp64 0-dim device tensors instead and nothing synchronises."""

    def __init__(self, balanced=True):
        super().__init__()
        self.balanced = balanced

    def forward(self, pred, gt, weight=None, device_stats: bool = False):
        loss, stats = _ClassificationFn.apply(pred, gt, weight, self.balanced, _wants_grad(pred))
        vals = stats if device_stats else stats.cpu().tolist()
        out = {"loss": loss}
        for i, name in enumerate(CLASSIFICATION_STATS[1:6], start=1):
            out[name] = vals[i]
        return out


class SpectralMatchingLoss(nn.Module):
    """libs/loss.py:115-139.  forward(M, gt_labels) -> fp32 0-dim device tensor, differentiable in M.
    from_features(normed, sigma, gt_labels): the same loss of the feature-similarity matrix the validation forward builds from
    `normed` and `sigma` (models/PointDSC.py:158-163), without the matrix being stored; differentiable in normed and sigma."""

    def __init__(self, balanced=True):
        super().__init__()
        self.balanced = balanced

    def forward(self, M, gt_labels):
        return _SmMatrixFn.apply(M, gt_labels, self.balanced, _wants_grad(M))

    def from_features(self, normed, sigma, gt_labels):
        return _SmFeaturesFn.apply(normed, sigma, gt_labels, self.balanced, _wants_grad(normed), _wants_grad(sigma))


class TransformationLoss(nn.Module):
    """libs/loss.py:12-63.  forward(trans, gt_trans, src_keypts, tgt_keypts, probs) ->
    (loss, recall, RE, TE, RMSE): fp32 0-dim device tensors, recall a Python float (one copy), as the reference returns them.
    The loss is differentiable in trans (rows 0..2) when trans requires a gradient and grad mode is on; otherwise no graph is
    built and no gradient kernel runs.  recall, RE, TE and RMSE never carry a graph.
    device_stats=True: recall, RE, TE and RMSE are fp64 0-dim device tensors and nothing synchronises.
    For bs > 1 the reference subtracts the whole [bs,N,3] target from every pair's warped source; that broadcast is mirrored."""

    def __init__(self, re_thre=15, te_thre=30):
        super().__init__()
        self.re_thre = re_thre
        self.te_thre = te_thre

    def forward(self, trans, gt_trans, src_keypts, tgt_keypts, probs, device_stats: bool = False):
        if _wants_grad(trans):
            loss, out = _TransformationFn.apply(trans, gt_trans, src_keypts, tgt_keypts, probs, self.re_thre, self.te_thre)
        else:
            out = transformation_loss_raw(trans, gt_trans, src_keypts, tgt_keypts, probs, self.re_thre, self.te_thre)
            loss = out[0].to(torch.float32)
        if device_stats:
            return loss, out[1], out[2], out[3], out[4]
        f32 = out.to(torch.float32)
        return loss, float(out[1].cpu()), f32[2], f32[3], f32[4]
