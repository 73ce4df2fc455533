"""The training path: the differentiable spatial-consistency attention (f-12), the reference's NonLocalBlock built on it, and
(f-13) the differentiable feature-similarity matrix, the train()-mode forward and ``TrainablePointDSC``.

Of the training path two operations need a hand-written backward: the attention (in torch it materialises bs x N x N scores twice
per layer) and the feature-similarity matrix M (its gradient for an arbitrary dM is a second N x N x 128 product behind a clamp
mask).  ``sc_attention`` is a ``torch.autograd.Function`` over ``ops.sc_attention_lse`` / ``ops.sc_attention_backward``;
``feature_similarity`` one over ``ops.feature_compat`` / ``ops.feature_compat_backward``; (f-14) ``seed_solve`` one over the per-seed
solver (``ops.seed_power_iteration`` + ``ops.seed_transforms`` / ``ops.seed_solve_backward``), which gives ``final_trans`` a
gradient.  The 1x1 convolutions, batch-norms and ReLUs around them are torch's by default; (f-16) ``linear_rows``,
``qkv_projection`` and ``classification_head`` are the plain linears of the train path (layer0, fc_message.6 with its residual,
the three projections in one launch, the head in one launch) over ``ops.linear_train_*`` / ``ops.qkv_train_*`` /
``ops.head_train_*``, which ``TrainablePointDSC(fused_linears=True)`` uses; (f-15) ``conv_bn_relu`` is the fused
train-mode Conv1d(k=1) + BatchNorm1d + ReLU over ``ops.pointwise_train_forward`` / ``ops.pointwise_train_backward``, which
``TrainablePointDSC(fused_layers=True)`` uses for the blocks' three such groups.  ``NonLocalBlock`` is the reference block
(models/PointDSC.py:9-45) for a trainer that swaps layer by layer; ``train_forward`` is the reference's whole forward without the
'testing' key (models/PointDSC.py:143-197) on a ``PointDSC`` module's own parameters, and ``TrainablePointDSC`` the module that
calls it in ``train()`` mode.  ``PointDSC.forward`` itself keeps refusing ``train()`` mode.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .model import PointDSC

CHANNELS = 128
# q rows enter the library pre-scaled: scores are taken in the log2 domain, p = exp2(compat * <q', k> - lse)
Q_SCALE = math.log2(math.e) / math.sqrt(CHANNELS)


def _pad_compat(compat: torch.Tensor, n: int) -> torch.Tensor:
    """compat [bs,N,N] or [bs,N,ld] -> [bs,N,ld'] with ld' a multiple of 4 and >= N rounded up to 32 (zero columns appended)."""
    ld = compat.shape[-1]
    need = (n + 31) // 32 * 32
    if ld >= need and ld % 4 == 0:
        return compat.contiguous()
    return torch.nn.functional.pad(compat, (0, max(need, (ld + 3) // 4 * 4) - ld)).contiguous()


class _SCAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, compat):
        bs, n, _ = q.shape
        qkv = torch.cat((q * Q_SCALE, k, v), dim=-1).reshape(bs * n, 3 * CHANNELS)
        msg, lse = ops.sc_attention_lse(qkv, compat, bs, n)
        ctx.save_for_backward(qkv, compat, msg, lse)
        ctx.shape = (bs, n)
        return msg.view(bs, n, CHANNELS)

    @staticmethod
    def backward(ctx, dmsg):
        qkv, compat, msg, lse = ctx.saved_tensors
        bs, n = ctx.shape
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return None, None, None, None
        dqkv = ops.sc_attention_backward(qkv, compat, msg, lse, dmsg.reshape(bs * n, CHANNELS).contiguous(), bs, n)
        dqkv = dqkv.view(bs, n, 3 * CHANNELS)
        dq = dqkv[..., :CHANNELS] * Q_SCALE if need_q else None
        dk = dqkv[..., CHANNELS:2 * CHANNELS] if need_k else None
        dv = dqkv[..., 2 * CHANNELS:] if need_v else None
        return dq, dk, dv, None


def sc_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, compat: torch.Tensor) -> torch.Tensor:
    """softmax_i(compat[o][i] <q_o, k_i> / sqrt(128)) v_i with gradients for q, k and v (models/PointDSC.py:39-42, one head).

    q, k, v [bs,N,128] un-scaled fp32; compat [bs,N,N] or [bs,N,ld] fp32 -> [bs,N,128].  compat gets no gradient (the reference
    builds it under no_grad): one that requires grad is refused rather than silently given None."""
    if compat.requires_grad:
        raise ValueError("sc_attention: compat gets no gradient (the reference builds it under no_grad); detach it")
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (compat, "compat")):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if q.dim() != 3 or q.shape[-1] != CHANNELS or k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"sc_attention: q, k, v must be [bs,N,{CHANNELS}] alike, got {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    bs, n, _ = q.shape
    if compat.dim() != 3 or compat.shape[0] != bs or compat.shape[1] != n or compat.shape[2] < n:
        raise ValueError(f"sc_attention: compat must be [bs,N,N] or [bs,N,ld >= N], got {tuple(compat.shape)}")
    return _SCAttention.apply(q, k, v, _pad_compat(compat, n))


class NonLocalBlock(nn.Module):
    """The reference's NonLocalBlock (models/PointDSC.py:9-45) for training: torch Conv1d / BatchNorm1d / ReLU with the reference's
    parameter names (a slice of its state_dict loads with strict=True) and ``sc_attention`` in place of the two einsums and the
    softmax.  One head of 128 channels is what the kernels are built for; anything else is refused."""

    def __init__(self, num_channels: int = CHANNELS, num_heads: int = 1):
        super().__init__()
        if num_channels != CHANNELS or num_heads != 1:
            raise ValueError(f"NonLocalBlock supports num_channels={CHANNELS}, num_heads=1 only (got {num_channels}, {num_heads})")
        self.fc_message = nn.Sequential(
            nn.Conv1d(num_channels, num_channels // 2, kernel_size=1),
            nn.BatchNorm1d(num_channels // 2),
            nn.ReLU(inplace=True),
            nn.Conv1d(num_channels // 2, num_channels // 2, kernel_size=1),
            nn.BatchNorm1d(num_channels // 2),
            nn.ReLU(inplace=True),
            nn.Conv1d(num_channels // 2, num_channels, kernel_size=1),
        )
        self.projection_q = nn.Conv1d(num_channels, num_channels, kernel_size=1)
        self.projection_k = nn.Conv1d(num_channels, num_channels, kernel_size=1)
        self.projection_v = nn.Conv1d(num_channels, num_channels, kernel_size=1)
        self.num_channels = num_channels
        self.head = num_heads

    def forward(self, feat: torch.Tensor, attention: torch.Tensor) -> torch.Tensor:
        """feat [bs,128,N], attention (the spatial-consistency matrix) [bs,N,N] or [bs,N,ld] -> [bs,128,N]."""
        q = self.projection_q(feat).transpose(1, 2)
        k = self.projection_k(feat).transpose(1, 2)
        v = self.projection_v(feat).transpose(1, 2)
        message = sc_attention(q.contiguous(), k.contiguous(), v.contiguous(), attention).transpose(1, 2)
        return feat + self.fc_message(message)


# ---------------------------------------------------------------------------------------------------------------------------
# f-13: the differentiable M, the train()-mode forward
# ---------------------------------------------------------------------------------------------------------------------------
class _SCAttentionRows(torch.autograd.Function):
    """_SCAttention on rows as the library takes them: qkv [bs*N,384] = (q | k | v) with q pre-scaled, as ONE GEMM with the
    concatenated weights leaves them -- no cat and no transposes of activations; the gradient is the one with respect to these rows
    (the q scale lives in the weights, where autograd finds it)."""

    @staticmethod
    def forward(ctx, qkv, compat, bs, n):
        msg, lse = ops.sc_attention_lse(qkv, compat, bs, n)
        ctx.save_for_backward(qkv, compat, msg, lse)
        ctx.shape = (bs, n)
        return msg

    @staticmethod
    def backward(ctx, dmsg):
        qkv, compat, msg, lse = ctx.saved_tensors
        bs, n = ctx.shape
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return ops.sc_attention_backward(qkv, compat, msg, lse, dmsg.contiguous(), bs, n), None, None, None


class _FeatureSimilarity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normed, sigma):
        bs, n, _ = normed.shape
        ctx.save_for_backward(normed, sigma)                  # no N x N tensor is kept: the backward recomputes the mask
        return ops.feature_compat(normed.reshape(bs * n, CHANNELS), sigma, bs, n)

    @staticmethod
    def backward(ctx, dM):
        normed, sigma = ctx.saved_tensors
        bs, n, _ = normed.shape
        need_n, need_s = ctx.needs_input_grad
        if not (need_n or need_s):
            return None, None
        dn, ds = ops.feature_compat_backward(normed.reshape(bs * n, CHANNELS), sigma, dM, bs, n, want_dnormed=need_n, want_dsigma=need_s)
        return (dn.view(bs, n, CHANNELS) if need_n else None), (ds.to(torch.float32).reshape(sigma.shape) if need_s else None)


def feature_similarity(normed: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    """M = clamp(1 - (1 - F F^T) / sigma^2, 0, 1) with a zero diagonal (models/PointDSC.py:160-163), with gradients for the
    features and sigma.  normed [bs,N,128] fp32 (unit rows), sigma one fp32 value -> M [bs,N,N], bit for bit ops.feature_compat's."""
    for t, name in ((normed, "normed"), (sigma, "sigma")):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if normed.dim() != 3 or normed.shape[-1] != CHANNELS:
        raise ValueError(f"feature_similarity: normed must be [bs,N,{CHANNELS}], got {tuple(normed.shape)}")
    if sigma.numel() != 1:
        raise ValueError(f"feature_similarity: sigma must hold one value, got {tuple(sigma.shape)}")
    return _FeatureSimilarity.apply(normed.contiguous(), sigma)


# ---------------------------------------------------------------------------------------------------------------------------
# f-14: the differentiable per-seed solver
# ---------------------------------------------------------------------------------------------------------------------------
class _SeedSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normed, sigma, src, tgt, knn_idx, sigma_spat, num_iterations):
        bs = src.shape[0]
        iters, mask, _ = ops.seed_power_iteration(normed, src, tgt, knn_idx, sigma, sigma_spat, num_iterations)
        if bs > 1:
            # the reference takes the power iteration's early exit over the seeds of ALL pairs (one allclose over [bs*S, k])
            _lib.check(_lib.load().pdsc_conv_mask_all_pairs(ops._p(mask), bs, ops._stream()), "pdsc_conv_mask_all_pairs")
        seed_trans, _ = ops.seed_transforms(src, tgt, knn_idx, iters, mask, num_iterations)
        ctx.save_for_backward(normed, sigma, src, tgt, knn_idx, sigma_spat, mask)       # the iterates are replayed, not kept
        ctx.num_iterations = num_iterations
        return seed_trans

    @staticmethod
    def backward(ctx, d_seed_trans):
        normed, sigma, src, tgt, knn_idx, sigma_spat, mask = ctx.saved_tensors
        need_n, need_s = ctx.needs_input_grad[:2]
        if not (need_n or need_s):
            return (None,) * 7
        dn, ds = ops.seed_solve_backward(normed, src, tgt, knn_idx, sigma, sigma_spat, mask, ctx.num_iterations,
                                         d_seed_trans.contiguous(), want_dnormed=need_n, want_dsigma=need_s)
        return (dn if need_n else None), (ds.to(torch.float32).reshape(sigma.shape) if need_s else None), None, None, None, None, None


def seed_solve(normed: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor, knn_idx: torch.Tensor, sigma: torch.Tensor,
               sigma_spat: torch.Tensor, num_iterations: int) -> torch.Tensor:
    """cal_seed_trans (models/PointDSC.py:248-320) with gradients for the features and sigma: the seeds' k x k feature * spatial
    matrices, the power iteration (the reference's early exit over all pairs included) and the weighted Procrustes.
    normed [bs,N,128], src, tgt [bs,N,3] fp32, knn_idx [bs,S,k] int32 (k <= 64), sigma, sigma_spat one fp32 value each ->
    seed_trans [bs,S,4,4], bit for bit ops.seed_power_iteration + ops.seed_transforms.  src, tgt, sigma_spat and knn_idx get no
    gradient: one of them that requires grad is refused rather than silently given None."""
    for t, name in ((src, "src"), (tgt, "tgt"), (sigma_spat, "sigma_spat")):
        if t.requires_grad:
            raise ValueError(f"seed_solve: {name} gets no gradient (only the features and sigma do); detach it")
    for t, name in ((normed, "normed"), (src, "src"), (tgt, "tgt"), (knn_idx, "knn_idx"), (sigma, "sigma"), (sigma_spat, "sigma_spat")):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
        want = torch.int32 if name == "knn_idx" else torch.float32
        if t.dtype != want:
            raise TypeError(f"{name} must be {want}, got {t.dtype}")
    if src.dim() != 3 or src.shape[-1] != 3 or tgt.shape != src.shape:
        raise ValueError(f"seed_solve: src and tgt must be [bs,N,3] alike, got {tuple(src.shape)} {tuple(tgt.shape)}")
    bs, n, _ = src.shape
    if normed.shape != (bs, n, CHANNELS):
        raise ValueError(f"seed_solve: normed must be [bs,N,{CHANNELS}], got {tuple(normed.shape)}")
    if knn_idx.dim() != 3 or knn_idx.shape[0] != bs or knn_idx.shape[1] < 1:
        raise ValueError(f"seed_solve: knn_idx must be [bs,S,k], got {tuple(knn_idx.shape)}")
    if not 1 <= knn_idx.shape[2] <= 64:
        raise ValueError(f"seed_solve: k = {knn_idx.shape[2]} neighbours per seed (1 .. 64)")
    if sigma.numel() != 1 or sigma_spat.numel() != 1:
        raise ValueError("seed_solve: sigma and sigma_spat must hold one value each")
    if not 0 <= int(num_iterations) <= 32:
        raise ValueError(f"seed_solve: num_iterations = {num_iterations} (0 .. 32)")
    return _SeedSolve.apply(normed.contiguous(), sigma, src.contiguous(), tgt.contiguous(), knn_idx.contiguous(), sigma_spat,
                            int(num_iterations))


# ---------------------------------------------------------------------------------------------------------------------------
# f-15: the fused train-mode point-wise layer
# ---------------------------------------------------------------------------------------------------------------------------
class _ConvBnRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bn_weight, bn_bias, running_mean, running_var, momentum, eps):
        z, y, mean, invstd = ops.pointwise_train_forward(x, weight, bias, bn_weight, bn_bias, running_mean, running_var, momentum, eps)
        ctx.save_for_backward(x, weight, bn_weight, bn_bias, y, mean, invstd)      # z is not kept: the mask is rebuilt from y
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz):
        x, weight, bn_weight, bn_bias, y, mean, invstd = ctx.saved_tensors
        need = ctx.needs_input_grad[:5]
        if not any(need):
            return (None,) * 9
        grads = ops.pointwise_train_backward(x, weight, bn_weight, bn_bias, y, mean, invstd, dz.contiguous(), *need)
        return (*grads, None, None, None, None)


def conv_bn_relu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, bn_weight: torch.Tensor, bn_bias: torch.Tensor,
                 running_mean: torch.Tensor, running_var: torch.Tensor, momentum: float = 0.1, eps: float = 1e-5) -> torch.Tensor:
    """relu(batch_norm(x weight^T + bias)) with BATCH statistics, on rows, in three device launches forward and four backward
    (Conv1d(k=1) -> BatchNorm1d -> ReLU of models/PointDSC.py:12-23,54-61 in train() mode), with gradients for x, weight, bias,
    bn_weight and bn_bias; only those that require grad are computed.
    x [M,Cin] fp32, weight [Cout,Cin] or the Conv1d's [Cout,Cin,1], the rest [Cout]; (Cin, Cout) one of (128,128), (128,64),
    (64,64); M >= 2 -> z [M,Cout].  running_mean and running_var are updated IN PLACE as F.batch_norm(training=True) does
    (momentum, unbiased variance); they get no gradient: one that requires grad is refused rather than silently given None."""
    for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t.requires_grad:
            raise ValueError(f"conv_bn_relu: {name} gets no gradient (it is a running statistic, updated in place); detach it")
    tensors = ((x, "x"), (weight, "weight"), (bias, "bias"), (bn_weight, "bn_weight"), (bn_bias, "bn_bias"),
               (running_mean, "running_mean"), (running_var, "running_var"))
    for t, name in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if weight.dim() == 3 and weight.shape[2] == 1:
        weight = weight[:, :, 0]
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"conv_bn_relu: x must be [M,Cin] and weight [Cout,Cin] or [Cout,Cin,1], got {tuple(x.shape)} {tuple(weight.shape)}")
    m, cin, cout = x.shape[0], x.shape[1], weight.shape[0]
    if (cin, cout) not in ops.POINTWISE_TRAIN_SHAPES:
        raise ValueError(f"conv_bn_relu: (Cin, Cout) = ({cin}, {cout}); supported: {ops.POINTWISE_TRAIN_SHAPES}")
    if m < 2:
        raise ValueError(f"conv_bn_relu: M = {m} rows (batch statistics need at least 2 values per channel)")
    for t, name in tensors[2:]:
        if t.shape != (cout,):
            raise ValueError(f"conv_bn_relu: {name} must be [{cout}], got {tuple(t.shape)}")
    if not (running_mean.is_contiguous() and running_var.is_contiguous()):
        raise ValueError("conv_bn_relu: running_mean and running_var must be contiguous (they are updated in place)")
    if not 0.0 <= float(momentum) <= 1.0 or float(eps) < 0.0:
        raise ValueError(f"conv_bn_relu: momentum = {momentum} (0 .. 1), eps = {eps} (>= 0)")
    for t, name in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    z = _ConvBnRelu.apply(x.contiguous(), weight.contiguous(), bias, bn_weight, bn_bias, running_mean, running_var, float(momentum),
                          float(eps))
    # the library wrote through the pointers: tell torch (the eval-mode module keys its packed weights on the version counters)
    torch.autograd.graph.increment_version(running_mean)
    torch.autograd.graph.increment_version(running_var)
    return z


# ---------------------------------------------------------------------------------------------------------------------------
# f-16: the train path's plain linears
# ---------------------------------------------------------------------------------------------------------------------------
def _weight2d(weight: torch.Tensor) -> torch.Tensor:
    """A Conv1d(k=1)'s [Cout,Cin,1] as [Cout,Cin] (a view: autograd hands the gradient back in the module's shape)."""
    return weight[:, :, 0] if weight.dim() == 3 and weight.shape[2] == 1 else weight


class _LinearRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        ctx.save_for_backward(x, weight)
        return ops.linear_train_forward(x, weight, bias, residual)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b, need_r = ctx.needs_input_grad
        dy = dy.contiguous()
        dx = dw = db = None
        if need_x or need_w or need_b:
            dx, dw, db = ops.linear_train_backward(x, weight, dy, need_x, need_w, need_b)
        return dx, dw, db, (dy if need_r else None)


def linear_rows(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor = None) -> torch.Tensor:
    """x weight^T + bias (+ residual) on rows, one device launch forward and up to three backward (a Conv1d(k=1) without a
    batch-norm: the encoder's layer0, and fc_message.6 with the block's ``feat + message``, models/PointDSC.py:45,68), with
    gradients for x, weight, bias and the residual; only those that require grad are computed.
    x [M,Cin] fp32, weight [128,Cin] or the Conv1d's [128,Cin,1], bias [128], residual [M,128] or None; Cin in 1 .. 16 or 64;
    M >= 1 -> [M,128]."""
    tensors = [(x, "x"), (weight, "weight"), (bias, "bias")] + ([(residual, "residual")] if residual is not None else [])
    for t, name in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    weight = _weight2d(weight)
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"linear_rows: x must be [M,Cin] and weight [Cout,Cin] or [Cout,Cin,1], got {tuple(x.shape)} {tuple(weight.shape)}")
    m, cin, cout = x.shape[0], x.shape[1], weight.shape[0]
    if not ops.linear_train_shape_ok(cin, cout):
        raise ValueError(f"linear_rows: (Cin, Cout) = ({cin}, {cout}); supported: (1..16, 128), (64, 128)")
    if m < 1:
        raise ValueError(f"linear_rows: M = {m} rows")
    if bias.shape != (cout,):
        raise ValueError(f"linear_rows: bias must be [{cout}], got {tuple(bias.shape)}")
    if residual is not None and residual.shape != (m, cout):
        raise ValueError(f"linear_rows: residual must be [{m},{cout}], got {tuple(residual.shape)}")
    for t, name in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    return _LinearRows.apply(x.contiguous(), weight.contiguous(), bias, None if residual is None else residual.contiguous())


class _QkvProjection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv):
        ctx.save_for_backward(x, wq, wk, wv)
        return ops.qkv_train_forward(x, wq, bq, wk, bk, wv, bv, Q_SCALE)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dqkv):
        x, wq, wk, wv = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need):
            return (None,) * 7
        return ops.qkv_train_backward(x, wq, wk, wv, Q_SCALE, dqkv.contiguous(), need)


def qkv_projection(x: torch.Tensor, wq: torch.Tensor, bq: torch.Tensor, wk: torch.Tensor, bk: torch.Tensor, wv: torch.Tensor,
                   bv: torch.Tensor) -> torch.Tensor:
    """The block's three projections in one launch (models/PointDSC.py:36-38): (Q_SCALE (x wq^T + bq) | x wk^T + bk | x wv^T + bv)
    as rows [M,384], the layout the attention takes, with gradients for x and the six UN-scaled parameters; no concatenated
    weight is built.  x [M,128] fp32, weights [128,128] or the Conv1d's [128,128,1], biases [128]."""
    tensors = ((x, "x"), (wq, "wq"), (bq, "bq"), (wk, "wk"), (bk, "bk"), (wv, "wv"), (bv, "bv"))
    for t, name in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    wq, wk, wv = _weight2d(wq), _weight2d(wk), _weight2d(wv)
    if x.dim() != 2 or x.shape[1] != CHANNELS or x.shape[0] < 1:
        raise ValueError(f"qkv_projection: x must be [M,{CHANNELS}] with M >= 1, got {tuple(x.shape)}")
    for t, name in ((wq, "wq"), (wk, "wk"), (wv, "wv")):
        if t.shape != (CHANNELS, CHANNELS):
            raise ValueError(f"qkv_projection: {name} must be [{CHANNELS},{CHANNELS}] or [{CHANNELS},{CHANNELS},1], got {tuple(t.shape)}")
    for t, name in ((bq, "bq"), (bk, "bk"), (bv, "bv")):
        if t.shape != (CHANNELS,):
            raise ValueError(f"qkv_projection: {name} must be [{CHANNELS}], got {tuple(t.shape)}")
    for t, name in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    return _QkvProjection.apply(x.contiguous(), wq.contiguous(), bq, wk.contiguous(), bk, wv.contiguous(), bv)


class _ClassificationHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, w0, b0, w1, b1, w2, b2):
        ctx.save_for_backward(feat, w0, b0, w1, b1, w2)          # no hidden layer and no mask is kept: the backward recomputes both
        return ops.head_train_forward(feat, w0, b0, w1, b1, w2, b2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        need = ctx.needs_input_grad
        if not any(need):
            return (None,) * 7
        return ops.head_train_backward(*ctx.saved_tensors, dlogits.contiguous(), need)


def classification_head(feat: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                        b2: torch.Tensor) -> torch.Tensor:
    """The classification head on rows (models/PointDSC.py:124-130,171): relu(relu(feat w0^T + b0) w1^T + b1) . w2 + b2 in one
    launch, logits [M], with gradients for feat and the six parameters.  feat [M,128] fp32, w0 [32,128], w1 [32,32], w2 [1,32] (or
    the Conv1d's three-dimensional weights), b0, b1 [32], b2 [1]."""
    tensors = ((feat, "feat"), (w0, "w0"), (b0, "b0"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"))
    for t, name in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    w0, w1, w2 = _weight2d(w0), _weight2d(w1), _weight2d(w2)
    hd = ops.HEAD_HIDDEN
    if feat.dim() != 2 or feat.shape[1] != CHANNELS or feat.shape[0] < 1:
        raise ValueError(f"classification_head: feat must be [M,{CHANNELS}] with M >= 1, got {tuple(feat.shape)}")
    for t, shape, name in ((w0, (hd, CHANNELS), "w0"), (b0, (hd,), "b0"), (w1, (hd, hd), "w1"), (b1, (hd,), "b1"), (w2, (1, hd), "w2"),
                           (b2, (1,), "b2")):
        if t.shape != shape:
            raise ValueError(f"classification_head: {name} must be {list(shape)}, got {tuple(t.shape)}")
    for t, name in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    return _ClassificationHead.apply(feat.contiguous(), w0.contiguous(), b0, w1.contiguous(), b1, w2.contiguous(), b2)


def _conv_rows(conv: nn.Conv1d, x: torch.Tensor) -> torch.Tensor:
    """A 1x1 Conv1d on channel-last rows [M, Cin] -> [M, Cout]."""
    return F.linear(x, conv.weight[:, :, 0], conv.bias)


def _conv_bn_relu_rows(conv: nn.Conv1d, bn: nn.BatchNorm1d, x: torch.Tensor, fused: bool) -> torch.Tensor:
    """Conv1d(k=1) -> BatchNorm1d -> ReLU on rows.  fused: one ``conv_bn_relu`` on the modules' own parameters and buffers, with
    num_batches_tracked incremented as BatchNorm1d.forward does; a batch-norm without running statistics or with momentum=None (a
    cumulative average, which the kernel does not compute) keeps torch's path, as does fused=False."""
    if not fused or not bn.track_running_stats or bn.momentum is None or bn.running_mean is None or not bn.affine:
        return F.relu(bn(_conv_rows(conv, x)))
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return conv_bn_relu(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)


def _linear_rows_fusable(conv: nn.Conv1d) -> bool:
    """A convolution the device linears take: it has a bias and its (Cin, Cout) is one of ``linear_rows``'."""
    return conv.bias is not None and ops.linear_train_shape_ok(conv.in_channels, conv.out_channels)


def _qkv_rows(nl, feat: torch.Tensor, fused: bool) -> torch.Tensor:
    """The block's q | k | v rows [M,384], q pre-scaled.  fused: ``qkv_projection`` on the three modules' own parameters; torch's
    path (one F.linear on concatenated weights) otherwise, and when a projection has no bias."""
    q, k, v = nl.projection_q, nl.projection_k, nl.projection_v
    if fused and q.bias is not None and k.bias is not None and v.bias is not None:
        return qkv_projection(feat, q.weight, q.bias, k.weight, k.bias, v.weight, v.bias)
    w = torch.cat((q.weight[:, :, 0] * Q_SCALE, k.weight[:, :, 0], v.weight[:, :, 0]))
    b = torch.cat((q.bias * Q_SCALE, k.bias, v.bias))
    return F.linear(feat, w, b)


def _head_rows(cls, feat: torch.Tensor, fused: bool) -> torch.Tensor:
    """The classification head's logits [M].  fused: ``classification_head``; torch's three F.linear otherwise, and when one of
    its convolutions has no bias."""
    if fused and all(cls[i].bias is not None for i in (0, 2, 4)):
        return classification_head(feat, cls[0].weight, cls[0].bias, cls[2].weight, cls[2].bias, cls[4].weight, cls[4].bias)
    return _conv_rows(cls[4], F.relu(_conv_rows(cls[2], F.relu(_conv_rows(cls[0], feat))))).reshape(-1)


def _train_encoder(enc, x: torch.Tensor, compat: torch.Tensor, bs: int, n: int, fused_layers: bool = False,
                   fused_linears: bool = False) -> torch.Tensor:
    """NonLocalNet.forward (models/PointDSC.py:65-77) on rows [bs*N, C].  The batch-norms are the modules' own forward on (M, C)
    rows (BatchNorm1d takes that layout: the statistics run over the bs * N rows exactly as over [bs, C, N]): F.batch_norm on
    the module's buffers with batch statistics, running_mean / running_var / num_batches_tracked updated by torch itself.
    fused_layers: the three conv + batch-norm + ReLU groups of every block run through ``conv_bn_relu`` instead (f-15); layer0,
    the q|k|v projection, fc_message.6 with its residual stay torch's unless
    fused_linears (f-16): layer0 and fc_message.6 + residual run through ``linear_rows``, the projection through
    ``qkv_projection`` (no cat of weights).  A convolution without a bias, or a layer0 whose in_dim is outside 1 .. 16, keeps
    torch's path."""
    if fused_linears and _linear_rows_fusable(enc.layer0):
        feat = linear_rows(x, enc.layer0.weight, enc.layer0.bias)
    else:
        feat = _conv_rows(enc.layer0, x)
    for i in range(enc.num_layers):
        pcn, nl = enc.blocks[f"PointCN_layer_{i}"], enc.blocks[f"NonLocal_layer_{i}"]
        feat = _conv_bn_relu_rows(pcn[0], pcn[1], feat, fused_layers)
        msg = _SCAttentionRows.apply(_qkv_rows(nl, feat, fused_linears), compat, bs, n)
        fc = nl.fc_message
        h = _conv_bn_relu_rows(fc[0], fc[1], msg, fused_layers)
        h = _conv_bn_relu_rows(fc[3], fc[4], h, fused_layers)
        if fused_linears and _linear_rows_fusable(fc[6]):
            feat = linear_rows(h, fc[6].weight, fc[6].bias, feat)
        else:
            feat = feat + _conv_rows(fc[6], h)
    return feat


def train_forward(model: PointDSC, data, differentiable_trans: bool = False, fused_layers: bool = False, *,
                  fused_linears: bool = False) -> dict:
    """The reference's forward without the 'testing' key (models/PointDSC.py:143-197) in train() mode, on `model`'s own Parameters
    and buffers: batch-statistics batch-norm (running statistics updated as torch's BatchNorm1d does), autograd through the
    encoder, the classification head and M.  data: corr_pos [bs,N,in_dim], src_keypts, tgt_keypts [bs,N,3] on the GPU.
    -> {'final_trans': the best seed hypothesis [bs,4,4], 'final_labels': the logits [bs,N], 'M': [bs,N,N]}.
    The spatial-consistency matrix, the seeds, their neighbours and the vote carry no gradient, as in the reference, and run as the
    library's stage ops.  differentiable_trans=False: neither do the power iteration and the Procrustes -- final_trans has no
    gradient and nothing is kept for one.  True: they run behind ``seed_solve`` and final_trans carries the gradient of the winning
    seed of each pair into the features and sigma (the reference's cal_seed_trans under autograd); the values are the same.
    fused_layers=True: every Conv1d + BatchNorm1d + ReLU group of the encoder's blocks runs as ``conv_bn_relu`` (device kernels,
    forward and backward) instead of torch's F.linear / F.batch_norm / F.relu: the same function, other rounding.
    fused_linears=True (keyword only, independent of fused_layers): the remaining plain linears -- layer0, every block's q|k|v
    projection and fc_message.6 with its residual, the classification head -- run as ``linear_rows``, ``qkv_projection`` and
    ``classification_head`` (device kernels, forward and backward) instead of F.linear / cat / relu: likewise."""
    if not model.training:
        raise RuntimeError("train_forward needs the module in train() mode; in eval() mode call the module (PointDSC.forward)")
    if "testing" in data.keys():
        raise ValueError("the 'testing' key belongs to eval() mode: the reference never runs its testing forward in train() mode")
    corr_pos, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
    for t, name in ((corr_pos, "corr_pos"), (src, "src_keypts"), (tgt, "tgt_keypts")):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on the GPU (pointdsc_amd has no CPU path)")
    dev = corr_pos.device
    corr_pos = corr_pos.detach().to(torch.float32).contiguous()
    src = src.detach().to(device=dev, dtype=torch.float32).contiguous()
    tgt = tgt.detach().to(device=dev, dtype=torch.float32).contiguous()
    bs, n = corr_pos.shape[0], corr_pos.shape[1]
    if corr_pos.shape[2] != model.in_dim or src.shape != (bs, n, 3) or tgt.shape != (bs, n, 3):
        raise ValueError("bad input shapes for train_forward")
    num_seeds, k = int(n * model.ratio), min(model.k, n - 1)
    if num_seeds < 1 or k < 1:
        raise ValueError(f"train_forward needs int(N * ratio) >= 1 seeds and N >= 2 (N = {n}, ratio = {model.ratio})")
    with torch.cuda.device(dev):
        with torch.no_grad():
            compat = _pad_compat(ops.spatial_compat(src, tgt, model.sigma_spat), n)
        feat = _train_encoder(model.encoder, corr_pos.view(bs * n, model.in_dim), compat, bs, n, fused_layers=fused_layers,
                              fused_linears=fused_linears)
        normed = F.normalize(feat, p=2, dim=-1).view(bs, n, CHANNELS)
        cls = model.classification
        logits = _head_rows(cls, feat, fused_linears).view(bs, n)
        M = feature_similarity(normed, model.sigma)
        with torch.no_grad():
            nd, sigma = normed.detach(), model.sigma.detach()
            seeds = ops.rank_select(logits.detach().contiguous(), num_seeds)          # argsort(logits, descending)[:, :num_seeds]
            knn_idx = ops.knn_seeds(nd, seeds, k, form="matrix")
        if differentiable_trans:
            # the same launches behind an autograd.Function; the winner gathered with the vote's own index, so final_trans carries
            # the gradient of one seed per pair (models/PointDSC.py:325-335: the reference indexes seed_trans with argmax too)
            seed_trans = seed_solve(normed, src, tgt, knn_idx, model.sigma, model.sigma_spat.detach(), model.num_iterations)
            with torch.no_grad():
                best = ops.score_hypotheses(seed_trans.detach(), src, tgt, float(model.inlier_threshold))[1]
            final_trans = seed_trans[torch.arange(bs, device=dev), best.long()]
        else:
            with torch.no_grad():
                iters, mask, _ = ops.seed_power_iteration(nd, src, tgt, knn_idx, sigma, model.sigma_spat, model.num_iterations)
                if bs > 1:
                    # the reference takes the power iteration's early exit over the seeds of ALL pairs (one allclose over [bs*S, k])
                    _lib.check(_lib.load().pdsc_conv_mask_all_pairs(ops._p(mask), bs, ops._stream()), "pdsc_conv_mask_all_pairs")
                seed_trans, _ = ops.seed_transforms(src, tgt, knn_idx, iters, mask, model.num_iterations)
                final_trans = ops.score_hypotheses(seed_trans, src, tgt, float(model.inlier_threshold))[2]
    return {"final_trans": final_trans, "final_labels": logits, "M": M}


class TrainablePointDSC(PointDSC):
    """``PointDSC`` a trainer can hold: the same constructor, parameters and 358-key state_dict (strict loading both ways).
    In ``train()`` mode ``forward`` is ``train_forward`` (batch statistics, autograd; the reference's Trainer.train_epoch,
    libs/trainer.py:79-136, runs on it unchanged); in ``eval()`` mode it is ``PointDSC.forward``, which sees every optimiser step
    through the weights' version counters.  ``differentiable_trans=True`` (keyword only, not part of the reference's constructor):
    the train-mode ``final_trans`` carries a gradient (``train_forward``), what a transformation-loss weight above 0 needs.
    ``fused_layers=True`` (keyword only, likewise): the blocks' conv + batch-norm + ReLU groups run as ``conv_bn_relu``.
    ``fused_linears=True`` (keyword only, likewise, independent of ``fused_layers``): layer0, the q|k|v projections, fc_message.6
    with its residual and the classification head run as ``linear_rows``, ``qkv_projection`` and ``classification_head``."""

    def __init__(self, *args, differentiable_trans: bool = False, fused_layers: bool = False, fused_linears: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.differentiable_trans = bool(differentiable_trans)
        self.fused_layers = bool(fused_layers)
        self.fused_linears = bool(fused_linears)

    def forward(self, data):
        if self.training:
            return train_forward(self, data, differentiable_trans=self.differentiable_trans, fused_layers=self.fused_layers,
                                 fused_linears=self.fused_linears)
        return super().forward(data)
