"""fp64 oracle of the spatial-consistency attention and its backward (include/pointdsc_hip.h section f-12), in plain torch.

One pair, C = 128, queries o, keys i:  c = compat[o][i],  z = <q_o, k_i> / sqrt(C),  s = c z,  P = softmax_i(s),  O_o = sum_i P_oi v_i.
Dense softmax: entries with c == 0 contribute exp(0).  Given dO:

    D_o   = <dO_o, O_o>              dV_i = sum_o P_oi dO_o            dP_oi = <dO_o, v_i>
    dS_oi = P_oi (dP_oi - D_o)       dZ_oi = c_oi dS_oi
    dQ_o  = sum_i dZ_oi k_i / sqrt(C)                                   dK_i = sum_o dZ_oi q_o / sqrt(C)

`closed_form` is these lines; `reference_lines` is the forward the reference block computes (models/PointDSC.py:39-42, one head),
which torch autograd differentiates: the CPU tests hold the two to rtol 1e-12 in fp64, and the fp32 autograd of the same lines
is the yardstick `e32` of the device tests."""
import math

import numpy as np
import torch

C = 128
# bs, N: the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (1, 33),     # one key past a full tile, a partial query block, a one-key dKV tail
    (2, 100),    # batch stride, a partial block in both roles
    (1, 129),    # a second query block and a second key block holding one row
    (2, 257),    # an odd tile count, two pairs
    (1, 520),    # the forward's forced splits (lse from the one-pass epilogue and from the merge)
]
SCALES = [1, 3]  # flat softmax; peaked (logits to about +-40)
FLOOR = 128 * 2.0 ** -24     # gamma_128: the worst-case relative error of one 128-term fp32 dot product


def make_case(bs, n, scale):
    """fp32 q, k, v, dO ~ N(0,1) * scale [bs,n,128]; compat = clip(U(-0.5, 1), 0, 1) [bs,n,n] (about a third exact zeros, NOT
    symmetric) with a unit diagonal.  Seed 100 + n."""
    rs = np.random.RandomState(100 + n)
    t = {name: torch.from_numpy((rs.standard_normal((bs, n, C)) * scale).astype(np.float32)) for name in ("q", "k", "v", "dO")}
    compat = np.clip(rs.uniform(-0.5, 1.0, (bs, n, n)), 0.0, 1.0).astype(np.float32)
    compat[:, np.arange(n), np.arange(n)] = 1.0
    t["compat"] = torch.from_numpy(compat)
    return t


def reference_lines(q, k, v, compat):
    """[bs,n,C] x3, [bs,n,n] -> message [bs,n,C]: scores / sqrt(C), softmax of compat * scores over the keys, weighted values."""
    feat_attention = torch.matmul(q, k.transpose(1, 2)) / C ** 0.5
    weight = torch.softmax(compat * feat_attention, dim=-1)
    return torch.matmul(weight, v)


def closed_form(q, k, v, compat, dO):
    """The formulas of the module docstring -> dict msg, lse (log2 domain: log2 sum_i exp(s_oi)), dq, dk, dv."""
    s = compat * (torch.matmul(q, k.transpose(1, 2)) / math.sqrt(C))
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    P = e / l
    O = torch.matmul(P, v)
    D = (dO * O).sum(dim=-1, keepdim=True)
    dV = torch.matmul(P.transpose(1, 2), dO)
    dP = torch.matmul(dO, v.transpose(1, 2))
    dS = P * (dP - D)
    dZ = compat * dS
    dQ = torch.matmul(dZ, k) / math.sqrt(C)
    dK = torch.matmul(dZ.transpose(1, 2), q) / math.sqrt(C)
    return {"msg": O, "lse": ((m + torch.log(l)) / math.log(2.0)).squeeze(-1), "dq": dQ, "dk": dK, "dv": dV}


def autograd_lines(q, k, v, compat, dO):
    """torch autograd of reference_lines in the dtype of the inputs -> dict msg, dq, dk, dv."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    msg = reference_lines(q, k, v, compat)
    dq, dk, dv = torch.autograd.grad(msg, (q, k, v), dO)
    return {"msg": msg.detach(), "dq": dq, "dk": dk, "dv": dv}


def err(x, x64):
    """max|X - X64| / max|X64|"""
    return float((x.to(torch.float64) - x64).abs().max() / x64.abs().max())


def oracle(case):
    """fp64 closed form on the fp32 inputs of `case`."""
    return closed_form(*(case[name].to(torch.float64) for name in ("q", "k", "v", "compat", "dO")))


def e32(case, ref64):
    """The yardstick: err of torch's own fp32 autograd of the reference lines on the CPU, maximum over msg, dq, dk, dv."""
    got = autograd_lines(*(case[name] for name in ("q", "k", "v", "compat", "dO")))
    return max(err(got[name], ref64[name]) for name in ("msg", "dq", "dk", "dv"))


def bound(e32_value):
    """err <= max(4 e32, gamma_128): the device differs from torch's fp32 in summation order and in v_exp_f32 against libm only --
    the same error class; the floor keeps a lucky small e32 from failing a correct kernel."""
    return max(4.0 * e32_value, FLOOR)


class TorchBlock(torch.nn.Module):
    """The non-local block in plain torch with the formula attention (the parameter names of the reference block): what
    training.NonLocalBlock is checked against, in fp64 (the oracle) and in fp32 (the yardstick)."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.fc_message = nn.Sequential(nn.Conv1d(C, C // 2, 1), nn.BatchNorm1d(C // 2), nn.ReLU(), nn.Conv1d(C // 2, C // 2, 1),
                                        nn.BatchNorm1d(C // 2), nn.ReLU(), nn.Conv1d(C // 2, C, 1))
        self.projection_q = nn.Conv1d(C, C, 1)
        self.projection_k = nn.Conv1d(C, C, 1)
        self.projection_v = nn.Conv1d(C, C, 1)

    def forward(self, feat, compat):
        q, k, v = (p(feat).transpose(1, 2) for p in (self.projection_q, self.projection_k, self.projection_v))
        return feat + self.fc_message(reference_lines(q, k, v, compat).transpose(1, 2))


# the reference block's state_dict (models/PointDSC.py:9-25 at num_channels 128), spelled out: the reference tree is not on the GPU box
BLOCK_STATE = [
    ("fc_message.0.weight", (64, 128, 1)), ("fc_message.0.bias", (64,)),
    ("fc_message.1.weight", (64,)), ("fc_message.1.bias", (64,)), ("fc_message.1.running_mean", (64,)),
    ("fc_message.1.running_var", (64,)), ("fc_message.1.num_batches_tracked", ()),
    ("fc_message.3.weight", (64, 64, 1)), ("fc_message.3.bias", (64,)),
    ("fc_message.4.weight", (64,)), ("fc_message.4.bias", (64,)), ("fc_message.4.running_mean", (64,)),
    ("fc_message.4.running_var", (64,)), ("fc_message.4.num_batches_tracked", ()),
    ("fc_message.6.weight", (128, 64, 1)), ("fc_message.6.bias", (128,)),
    ("projection_q.weight", (128, 128, 1)), ("projection_q.bias", (128,)),
    ("projection_k.weight", (128, 128, 1)), ("projection_k.bias", (128,)),
    ("projection_v.weight", (128, 128, 1)), ("projection_v.bias", (128,)),
]
# a train-mode batch-norm removes any per-channel constant of its input.  The biases of the two convolutions in front of one add
# such a constant, and so does the value projection's bias (the softmax weights of a row sum to 1, so it reaches fc_message.0 as a
# constant and leaves through fc_message.1): their gradient is zero in exact arithmetic, what is computed is rounding noise.  Their
# error is therefore measured against the scale of the same convolution's weight gradient.
ZERO_GRAD_BIAS = {"fc_message.0.bias": "fc_message.0.weight", "fc_message.3.bias": "fc_message.3.weight",
                  "projection_v.bias": "projection_v.weight"}


def block_run(block, feat, compat, w):
    """loss = sum(block(feat, compat) * w) -> (output, {parameter name: gradient}) ; the block is left in train() mode."""
    block.train()
    block.zero_grad()
    out = block(feat, compat)
    (out * w).sum().backward()
    return out.detach(), {name: p.grad.detach().clone() for name, p in block.named_parameters()}


def block_errors(out, grads, out64, grads64):
    """err per tensor of a block run against the fp64 run (ZERO_GRAD_BIAS entries on their weight's scale)."""
    errs = {"out": err(out, out64)}
    for name, g64 in grads64.items():
        scale = grads64[ZERO_GRAD_BIAS.get(name, name)].abs().max()
        errs[name] = float((grads[name].to(torch.float64).cpu() - g64).abs().max() / scale)
    return errs
