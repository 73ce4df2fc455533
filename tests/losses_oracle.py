"""fp64 oracle of the device losses (pointdsc_amd/losses.py, include/pointdsc_hip.h section f-11): the formulas of the header
restated in plain torch, gradients by autograd.  Also the case table of tests/test_losses.py (inputs from numpy RandomState
streams, so every machine draws the same numbers) and the derived tolerances of the features form of the spectral-matching loss.
"""
from __future__ import annotations

import math

import numpy as np
import torch

K = 128                      # channels
F32_EPS = 2.0 ** -24         # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------------------
# formulas
# ---------------------------------------------------------------------------------------------------------------------------
def classification(pred, gt, weight=None, balanced=True):
    """pred, gt (, weight) [bs,N] fp64 -> dict: loss (0-dim, differentiable in pred), precision, recall, f1 (pair 0, pred > 0, zero
    where a denominator is zero), logit_true, logit_false (batch, denominators max(1, count)), num_pos, num_neg."""
    num_pos = torch.relu(gt.sum() - 1) + 1
    num_neg = torch.relu((1 - gt).sum() - 1) + 1
    l = torch.log1p(torch.exp(-pred.abs()))
    sp_pos, sp_neg = l + torch.clamp(pred, min=0), l + torch.clamp(-pred, min=0)          # softplus(x), softplus(-x)
    if weight is not None:
        loss = (((1 - gt) * sp_pos + gt * sp_neg) * weight).mean()
    elif not balanced:
        loss = ((1 - gt) * sp_pos + gt * sp_neg).mean()
    else:
        loss = ((1 - gt) * sp_pos + (num_neg / num_pos) * gt * sp_neg).mean()
    p0, g0 = pred[0].detach() > 0, gt[0] == 1
    tp, pp, gp = int((p0 & g0).sum()), int(p0.sum()), int(g0.sum())
    return {"loss": loss, "precision": tp / pp if pp else 0.0, "recall": tp / gp if gp else 0.0,
            "f1": 2.0 * tp / (pp + gp) if pp + gp else 0.0,
            "logit_true": float((pred.detach() * gt).sum() / max(1.0, float(gt.sum()))),
            "logit_false": float((pred.detach() * (1 - gt)).sum() / max(1.0, float((1 - gt).sum()))),
            "num_pos": float(num_pos), "num_neg": float(num_neg), "tp": tp, "pp": pp, "gp": gp}


def gt_matrix(gt):
    """[bs,N] -> [bs,N,N]: gt_i gt_j off the diagonal, 0 on it."""
    g = ((gt[:, None, :] + gt[:, :, None]) == 2).to(gt.dtype)
    return g * (1 - torch.eye(gt.shape[1], dtype=gt.dtype))[None]


def class_sizes(gt):
    """closed form of the class sizes per pair: P = relu(k (k - 1) - 1) + 1, Q = relu(N^2 - k (k - 1) - 1) + 1."""
    n = gt.shape[1]
    k = (gt == 1).sum(-1).to(torch.float64)
    kk = k * (k - 1)
    return torch.relu(kk - 1) + 1, torch.relu(n * n - kk - 1) + 1


def sm_pair_values(M, gt, balanced=True):
    gm = gt_matrix(gt)
    if balanced:
        P, Q = class_sizes(gt)
        return 0.5 * (((M - 1) ** 2) * gm).sum((-1, -2)) / P + 0.5 * ((M ** 2) * (1 - gm)).sum((-1, -2)) / Q
    return ((M - gm) ** 2).sum((-1, -2)) / (M.shape[1] * M.shape[2])


def sm_matrix(M, gt, balanced=True):
    return sm_pair_values(M, gt, balanced).mean()


def feature_raw(normed, sigma):
    """normed [bs,N,K] -> raw = 1 - (1 - F F^T) / sigma^2 and the Gram matrix s."""
    s = normed @ normed.transpose(1, 2)
    return 1 - (1 - s) / sigma ** 2, s


def feature_matrix(normed, sigma):
    raw, _ = feature_raw(normed, sigma)
    return torch.clamp(raw, 0, 1) * (1 - torch.eye(normed.shape[1], dtype=normed.dtype))[None]


def sm_features(normed, sigma, gt, balanced=True):
    return sm_matrix(feature_matrix(normed, sigma), gt, balanced)


def transformation(trans, gt_trans, src, tgt, probs, re_thre=15.0, te_thre=30.0):
    """fp64 inputs -> [loss, recall %, RE deg, TE cm, RMSE], means over the pairs.  The reference's broadcast is mirrored: pair i's
    warped source [N,3] is subtracted from the WHOLE target [bs,N,3].  The operations whose order matters to the last bit of an
    ill-conditioned result (the trace under the acos, the warp under the residual) are written out term by term."""
    bs = trans.shape[0]
    acc = [0.0] * 5
    for i in range(bs):
        R, G = trans[i, :3, :3], gt_trans[i, :3, :3]
        tr = torch.zeros((), dtype=torch.float64)
        for c in range(3):
            for r in range(3):
                tr = tr + R[r, c] * G[r, c]
        re = torch.acos(torch.clamp((tr - 1) / 2, -1, 1)) * 180 / math.pi
        d = trans[i, :3, 3] - gt_trans[i, :3, 3]
        te = torch.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * 100
        x, y, z = src[i, :, 0], src[i, :, 1], src[i, :, 2]
        sq = torch.zeros(tgt.shape[:2], dtype=torch.float64)
        for r in range(3):
            w = ((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + trans[i, r, 3]
            dd = w[None, :] - tgt[:, :, r]
            sq = sq + dd * dd
        acc[0] += float(sq.mean()) if bool((probs[i] > 0).any()) else 0.0
        acc[1] += 1.0 if (float(te) < te_thre and float(re) < re_thre) else 0.0
        acc[2] += float(re)
        acc[3] += float(te)
        acc[4] += float(torch.sqrt(sq).mean())
    return [acc[0] / bs, acc[1] * 100.0 / bs, acc[2] / bs, acc[3] / bs, acc[4] / bs]


# ---------------------------------------------------------------------------------------------------------------------------
# derived tolerances of the features form (fp32 Gram tiles against the fp64 oracle on the same fp32 features)
# ---------------------------------------------------------------------------------------------------------------------------
def delta(sigma: float) -> float:
    """bound on |M_device - M_oracle| per entry: a K-term fp32 dot product of unit vectors errs by at most K 2^-24, the few roundings
    of the clamp expression are covered by 8 more; the division by sigma^2 scales both."""
    return (K + 8) * F32_EPS / sigma ** 2


def value_bound(sigma: float) -> float:
    """|d loss / d M_ij| summed with its weights is at most 2, so |loss_device - loss_oracle| <= 2 delta."""
    return 2.0 * delta(sigma)


def loss_weights(gt, balanced=True):
    """c_ij [bs,N,N]: 0.5 / (P bs) on the positives, 0.5 / (Q bs) on the negatives; 1 / (bs N^2) unbalanced."""
    bs, n = gt.shape
    if not balanced:
        return torch.full((bs, n, n), 1.0 / (bs * n * n), dtype=torch.float64)
    P, Q = class_sizes(gt)
    gm = gt_matrix(gt)
    return gm * (0.5 / (P * bs))[:, None, None] + (1 - gm) * (0.5 / (Q * bs))[:, None, None]


def kink_entries(normed, sigma: float, gt) -> int:
    """Off-diagonal entries at which the loss gradient is discontinuous within the arithmetic's reach: a positive pair whose raw value
    is within 4 delta of 0 (the clamp switches its gradient -2c on), a negative pair within 4 delta of 1 (switches 2c off)."""
    raw, _ = feature_raw(normed, sigma)
    gm = gt_matrix(gt)
    off = 1 - torch.eye(gt.shape[1], dtype=torch.float64)[None]
    d = 4 * delta(sigma)
    bad = ((raw.abs() < d) & (gm == 1)) | (((raw - 1).abs() < d) & (gm == 0))
    return int((bad & (off == 1)).sum())


def dnormed_bound(gt, sigma: float, balanced, dnormed_oracle):
    """[bs,N] bound per row on every element of dF_i: an entry of g errs by at most c_ij 2 delta and |F_jc| <= 1, so the first product
    gives (2 / sigma^2) sum_j c_ij 2 delta; the second (fp32 MFMA) product adds K 2^-24 ||dF_i||_1."""
    c = loss_weights(gt, balanced)
    return (2.0 / sigma ** 2) * c.sum(-1) * 2 * delta(sigma) + K * F32_EPS * dnormed_oracle.abs().sum(-1)


def dsigma_bound(normed, sigma: float, gt, balanced) -> float:
    """dsigma = sum_ij g_ij 2 (1 - s_ij) / sigma^3: the error of g (c_ij 2 delta per entry) times its factor, the error of (1 - s_ij)
    ((K + 8) 2^-24) times |g_ij| 2 / sigma^3, and K 2^-24 of the sum of the magnitudes for the fp32 products and partial sums."""
    raw, s = feature_raw(normed, sigma)
    gm = gt_matrix(gt)
    c = loss_weights(gt, balanced)
    off = 1 - torch.eye(gt.shape[1], dtype=torch.float64)[None]
    g = c * 2 * (torch.clamp(raw, 0, 1) - gm) * ((raw >= 0) & (raw <= 1)) * off
    fac = (2 * (1 - s) / sigma ** 3).abs()
    return float((c * off * 2 * delta(sigma) * fac).sum() + (g.abs() * 2 * (K + 8) * F32_EPS / sigma ** 3).sum()
                 + K * F32_EPS * (g.abs() * fac).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# the case table: the smallest shapes at which the kernels can go wrong (N below, at, and above the 32-index tile and the 128-row
# block; one, two and three pairs) and every kind of label row
# ---------------------------------------------------------------------------------------------------------------------------
CASES = [
    {"n": 5, "labels": ["all"], "seed": 11},
    {"n": 37, "labels": ["none", "one"], "seed": 12},
    {"n": 64, "labels": ["some"], "seed": 13},
    {"n": 200, "labels": ["some", "all", "none"], "seed": 14},      # three column tiles of 64 and a remainder; two row blocks
]
SIGMAS = [0.8, 1.0, 1.3]
PERTURBATIONS = [(0.0, 0.0), (1.0, 0.02), (20.0, 0.5)]               # (degrees, metres)


def _labels(kind: str, n: int, rs) -> np.ndarray:
    if kind == "none":
        return np.zeros(n, np.float32)
    if kind == "all":
        return np.ones(n, np.float32)
    if kind == "one":
        g = np.zeros(n, np.float32)
        g[rs.randint(n)] = 1
        return g
    return (rs.random_sample(n) < 0.3).astype(np.float32)


def _rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def make_case(case: dict, case_index: int = 0) -> dict:
    """fp32 CPU tensors: pred, gt, weight [bs,N]; normed [bs,N,128]; trans, gt_trans [bs,4,4]; src, tgt [bs,N,3].
    Features: normalize(alpha gt_i c + noise) with alpha = 0.2 and noise = (+-1)^i d + 0.2 gaussian, c and d fixed unit directions: pairs of equal
    parity land inside (0, 1) of the clamp and pairs of opposite parity below 0 for every sigma of the table, inliers and outliers
    alike (so the all-inlier and the no-inlier rows reach both sides too).  Logits: normal scaled by 8 (both BCE tails).  Poses:
    the ground truth perturbed by PERTURBATIONS, cycling over the pairs.  Pair 1 of the second case has no positive logit."""
    rs = np.random.RandomState(case["seed"])
    n, bs = case["n"], len(case["labels"])
    gt = np.stack([_labels(kind, n, rs) for kind in case["labels"]])
    pred = (rs.standard_normal((bs, n)) * 8).astype(np.float32)
    if bs == 2:
        pred[1] = -np.abs(pred[1]) - 0.5
    weight = rs.random_sample((bs, n)).astype(np.float32)
    c, d = np.zeros(K), np.zeros(K)
    c[0], d[1] = 1.0, 1.0
    parity = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    f = 0.2 * gt[:, :, None] * c + parity[None, :, None] * d + 0.2 * rs.standard_normal((bs, n, K)) / np.sqrt(K)
    normed = torch.nn.functional.normalize(torch.from_numpy(f.astype(np.float32)), dim=-1)
    src = (rs.random_sample((bs, n, 3)) * 3).astype(np.float32)
    tgt = np.empty_like(src)
    gt_trans = np.tile(np.eye(4, dtype=np.float32), (bs, 1, 1))
    trans = gt_trans.copy()
    for b in range(bs):
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        t = rs.standard_normal(3) * 0.5
        gt_trans[b, :3, :3], gt_trans[b, :3, 3] = q, t
        warped = src[b] @ q.T.astype(np.float32) + t.astype(np.float32) + 0.01 * rs.standard_normal((n, 3)).astype(np.float32)
        rand = (rs.random_sample((n, 3)) * 3).astype(np.float32)
        tgt[b] = np.where(gt[b][:, None] == 1, warped, rand)
        deg, shift = PERTURBATIONS[(b + case_index) % 3]
        dR = _rotation(rs.standard_normal(3), deg)
        dt = rs.standard_normal(3)
        trans[b, :3, :3] = (dR @ q).astype(np.float32)
        trans[b, :3, 3] = (t + shift * dt / np.linalg.norm(dt)).astype(np.float32)
        if deg == 0.0:
            trans[b] = gt_trans[b]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    return {"pred": tt(pred), "gt": tt(gt), "weight": tt(weight), "normed": normed.contiguous(), "trans": tt(trans),
            "gt_trans": tt(gt_trans), "src": tt(src), "tgt": tt(tgt)}
