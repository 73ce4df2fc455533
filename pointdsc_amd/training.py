"""The differentiable spatial-consistency attention (f-12) and the reference's NonLocalBlock built on it.

Of the training path only the attention needs a hand-written backward: its 1x1 convolutions, batch-norms and ReLUs are operations
torch differentiates well, while the attention in torch materialises bs x N x N scores twice per layer.  ``sc_attention`` is a
``torch.autograd.Function`` over ``ops.sc_attention_lse`` / ``ops.sc_attention_backward``; ``NonLocalBlock`` is the reference block
(models/PointDSC.py:9-45) with torch layers around it, so a trainer can swap it in layer by layer.  ``PointDSC.forward`` in
``train()`` mode is not part of this.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops

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
