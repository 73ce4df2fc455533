"""Oracles of the training path's f-13 pieces (pointdsc_amd/training.py, include/pointdsc_hip.h section f-13), in plain torch.

A. The backward of the feature-similarity matrix M = clamp(1 - (1 - F F^T) / sigma^2, 0, 1) (zero diagonal) for an arbitrary dM:

    live_ij = (i != j) and 0 <= raw_ij <= 1       g_ij = live_ij ? dM_ij : 0
    dF_i    = (1 / sigma^2) sum_j (g_ij + g_ji) F_j
    dsigma  = (2 / sigma^3) sum_b sum_ij g_ij (1 - s_ij)

`closed_form` is these lines with `where`; `autograd_lines` differentiates the reference's three formula lines
(models/PointDSC.py:160-163); the CPU test holds the two to 1e-12 in fp64.  The case table and the DERIVED tolerances follow.

B. `TorchPointDSC`: the reference's train-mode forward (models/PointDSC.py:143-163,171) written fresh around
attention_backward_oracle.TorchBlock, generic in dtype, with the parameter names of the reference -- the truth (fp64, CPU) and
the yardstick (fp32, on the device) of tests/test_train_forward.py."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_backward_oracle as AO  # noqa: E402
import losses_oracle as LO  # noqa: E402

K, F32_EPS = LO.K, LO.F32_EPS

# ---------------------------------------------------------------------------------------------------------------------------
# A. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
# below, at and above the 32-index tile and the 128-row block; one to three pairs
CASES = list(LO.CASES) + [
    {"n": 33, "labels": ["some"], "seed": 17},
    {"n": 129, "labels": ["some"], "seed": 15},
    {"n": 257, "labels": ["some", "none"], "seed": 16},
]
SIGMAS = LO.SIGMAS
CASE_IDS = [f"N{c['n']}_bs{len(c['labels'])}" for c in CASES]


def make_case(i: int) -> dict:
    """LO.make_case of CASES[i] plus dM [bs,N,N]: seeded normal fp32, not symmetric."""
    c = LO.make_case(CASES[i], i)
    bs, n = c["gt"].shape
    rs = np.random.RandomState(5000 + CASES[i]["seed"])
    c["dM"] = torch.from_numpy(rs.standard_normal((bs, n, n)).astype(np.float32))
    return c


def kink_count(normed, sigma: float) -> int:
    """Off-diagonal entries whose fp64 raw lies within 4 delta(sigma) of 0 or of 1: there the fp32 mask may differ from the oracle's.
    Two-sided and independent of the labels (stricter than LO.kink_entries)."""
    raw, _ = LO.feature_raw(normed, sigma)
    off = ~torch.eye(normed.shape[1], dtype=torch.bool)[None]
    d = 4 * LO.delta(sigma)
    return int((((raw.abs() < d) | ((raw - 1).abs() < d)) & off).sum())


def live_mask(normed, sigma):
    raw, s = LO.feature_raw(normed, sigma)
    off = ~torch.eye(normed.shape[1], dtype=torch.bool)[None]
    return off & (raw >= 0) & (raw <= 1), s


def closed_form(normed, sigma, dM):
    """fp64 normed [bs,N,K], sigma (float or 0-dim), dM [bs,N,N] -> (dnormed [bs,N,K], dsigma float)."""
    live, s = live_mask(normed, sigma)
    g = torch.where(live, dM, torch.zeros_like(dM))
    dF = ((g + g.transpose(1, 2)) @ normed) / sigma ** 2
    return dF, float((2 / sigma ** 3) * (g * (1 - s)).sum())


def formula_lines(normed, sigma):
    """models/PointDSC.py:160-163."""
    M = torch.matmul(normed, normed.permute(0, 2, 1))
    M = torch.clamp(1 - (1 - M) / sigma ** 2, min=0, max=1)
    M = M.clone()
    M[:, torch.arange(M.shape[1]), torch.arange(M.shape[1])] = 0
    return M


def autograd_lines(normed, sigma, dM):
    """torch autograd of the formula lines in the dtype of the inputs -> (M, dnormed, dsigma 0-dim)."""
    normed = normed.detach().clone().requires_grad_(True)
    sg = torch.as_tensor(sigma, dtype=normed.dtype, device=normed.device).detach().clone().requires_grad_(True)
    M = formula_lines(normed, sg)
    dn, ds = torch.autograd.grad(M, (normed, sg), dM)
    return M.detach(), dn, ds


def dnormed_bound(normed, sigma: float, dM):
    """[bs,N] bound per row on every element of dF_i, derived as LO.dnormed_bound with |dM_ij| in place of the loss's coefficient.
    Under the kink condition (kink_count == 0) the first product's error, (K + 8) 2^-24 / sigma^2 = delta per raw, flips no mask
    entry, and -- unlike the loss, whose g depends on M -- g here IS dM where live: the first product adds nothing.  What remains
    is the second (fp32 MFMA) product, the one rounding of g_ij + g_ji and the scale by 1 / sigma^2: K 2^-24 of the magnitudes,
    (K 2^-24 / sigma^2) sum_j (|g_ij| + |g_ji|) with |F_jc| <= 1."""
    live, _ = live_mask(normed, sigma)
    g = torch.where(live, dM.abs(), torch.zeros_like(dM))
    return (K * F32_EPS / sigma ** 2) * (g.sum(-1) + g.sum(-2))


def dsigma_bound(normed, sigma: float, dM) -> float:
    """dsigma = (2 / sigma^3) sum g_ij (1 - s_ij), g exact under the kink condition: the error of (1 - s_ij) ((K + 8) 2^-24, the
    first product's error per s) times |g_ij| 2 / sigma^3, and K 2^-24 of the sum of the magnitudes for the fp32 products and the
    16-element fp32 partial sums (LO.dsigma_bound without its first term, the error of g)."""
    live, s = live_mask(normed, sigma)
    g = torch.where(live, dM.abs(), torch.zeros_like(dM))
    return float((g * 2 * (K + 8) * F32_EPS / sigma ** 3).sum() + K * F32_EPS * (g * (2 * (1 - s) / sigma ** 3).abs()).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# B. the whole model
# ---------------------------------------------------------------------------------------------------------------------------
class TorchPointDSC(torch.nn.Module):
    """The reference's train-mode forward up to (logits, M) in plain torch; parameter names as the reference's, so a PointDSC
    state_dict loads with strict=True."""

    def __init__(self, in_dim=6, num_layers=2):
        super().__init__()
        nn = torch.nn
        self.num_layers = num_layers
        self.sigma = nn.Parameter(torch.tensor([1.0]))
        self.sigma_spat = nn.Parameter(torch.tensor([0.1]), requires_grad=False)
        self.encoder = nn.Module()
        self.encoder.layer0 = nn.Conv1d(in_dim, AO.C, 1)
        self.encoder.blocks = nn.ModuleDict()
        for i in range(num_layers):
            self.encoder.blocks[f"PointCN_layer_{i}"] = nn.Sequential(nn.Conv1d(AO.C, AO.C, 1), nn.BatchNorm1d(AO.C), nn.ReLU())
            self.encoder.blocks[f"NonLocal_layer_{i}"] = AO.TorchBlock()
        self.classification = nn.Sequential(nn.Conv1d(AO.C, 32, 1), nn.ReLU(), nn.Conv1d(32, 32, 1), nn.ReLU(), nn.Conv1d(32, 1, 1))

    def forward(self, corr_pos, src, tgt):
        """-> (logits [bs,N], M [bs,N,N], normed [bs,N,C])"""
        with torch.no_grad():
            src_dist = torch.norm(src[:, :, None, :] - src[:, None, :, :], dim=-1)
            compat = src_dist - torch.norm(tgt[:, :, None, :] - tgt[:, None, :, :], dim=-1)
            compat = torch.clamp(1.0 - compat ** 2 / self.sigma_spat ** 2, min=0)
        feat = self.encoder.layer0(corr_pos.permute(0, 2, 1))
        for i in range(self.num_layers):
            feat = self.encoder.blocks[f"PointCN_layer_{i}"](feat)
            feat = self.encoder.blocks[f"NonLocal_layer_{i}"](feat, compat)
        normed = torch.nn.functional.normalize(feat.permute(0, 2, 1), p=2, dim=-1)
        M = formula_lines(normed, self.sigma)
        return self.classification(feat).squeeze(1), M, normed


def zero_grad_scales(names) -> dict:
    """{bias: weight of the same convolution} for the gradients that are ZERO in exact arithmetic, so that what is computed is
    rounding noise, measured on the scale of that convolution's weight gradient (f-12's rule, AO.ZERO_GRAD_BIAS).  A train-mode
    batch-norm removes any per-channel constant of its input, and a 1x1 convolution maps a constant to a constant:
      * inside a block: fc_message.0.bias, fc_message.3.bias, projection_v.bias (AO.ZERO_GRAD_BIAS);
      * PointCN_layer_i.0.bias: its own batch-norm follows;
      * encoder.layer0.bias and, for every block but the last, fc_message.6.bias: the constant they add to `feat` reaches nothing
        but the next PointCN convolution and leaves in its batch-norm (the last block's feeds the head: a real gradient)."""
    names = list(names)
    last = max(int(n.split("NonLocal_layer_")[1].split(".")[0]) for n in names if "NonLocal_layer_" in n)
    out = {}
    for n in names:
        if not n.endswith(".bias"):
            continue
        w = n[:-len("bias")] + "weight"
        if n == "encoder.layer0.bias" or ("PointCN_layer_" in n and n.endswith(".0.bias")):
            out[n] = w
        elif "NonLocal_layer_" in n:
            tail = n.split("NonLocal_layer_")[1].split(".", 1)[1]
            if tail in AO.ZERO_GRAD_BIAS or (tail == "fc_message.6.bias" and int(n.split("NonLocal_layer_")[1].split(".")[0]) < last):
                out[n] = w
    return out


def objective_run(model, corr_pos, src, tgt, W1, W2, forward=None):
    """L = <W1, logits> + <W2, M>, backward.  -> dict: logits, M, 'grad:<parameter>', 'buffer:<running statistic>' (detached,
    as the model holds them after the call).  `forward(model, corr_pos, src, tgt)` -> (logits, M) replaces model.__call__."""
    model.train()
    model.zero_grad()
    out = forward(model, corr_pos, src, tgt) if forward else model(corr_pos, src, tgt)
    logits, M = out[0], out[1]
    ((W1 * logits).sum() + (W2 * M).sum()).backward()
    res = {"logits": logits.detach(), "M": M.detach()}
    for name, p in model.named_parameters():
        if p.requires_grad:
            res["grad:" + name] = p.grad.detach().clone()
    for name, b in model.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            res["buffer:" + name] = b.detach().clone()
    return res


def errors(got: dict, ref64: dict) -> dict:
    """err(X) = max|X - X64| / max|X64| per tensor (zero-in-exact-arithmetic gradients on their weight gradient's scale)."""
    out = {}
    zero = zero_grad_scales(n[5:] for n in ref64 if n.startswith("grad:"))
    for name, x64 in ref64.items():
        scale = ref64["grad:" + zero[name[5:]] if name.startswith("grad:") and name[5:] in zero else name].abs().max()
        out[name] = float((got[name].detach().to(torch.float64).cpu() - x64).abs().max() / scale)
    return out


def bound(e32: float) -> float:
    return max(4.0 * e32, 128 * 2.0 ** -24)
