"""fp64 oracles of the evaluation side path (csrc/spectral.hip, csrc/metrics.hip) in plain torch, the fp32 yardsticks of the same
lines, the seeded cases and the bound -- shared by the CPU and the GPU part of tests/test_spectral_fp64.py.

    SM              M = max(0, 4.5 - d^2 / 2 / sigma^2), zero diagonal, d = |c_i[0:3] - c_j[0:3]| - |c_i[3:6] - c_j[3:6]|;
                    v = 1, iters x { v = M v; v /= |v| + 1e-6 };  labels = the num_top largest entries of v (ties by ascending index,
                    NaN the largest);  pose = rigid_transform_3d(src, tgt, v * labels)
    cal_confidence  the three formulas of the reference's PointDSC.cal_confidence, v NOT normalised
    eval row        the nine columns of ops.STATS_COLUMNS, NaN-propagating (torch.clamp keeps a NaN)

Every oracle takes the fp32 inputs cast to fp64.  The yardstick of a quantity X is the same lines in fp32 torch on the CPU (for SM:
oracle/sm_oracle.py), e32 = max|X32 - X64| / max|X64|, and a device result must lie within bound(e32, floor) = max(4 e32, floor) of
fp64: the device differs from torch's fp32 in summation order only -- the same error class; the floor keeps a lucky small e32 from
failing a correct kernel (the idiom of tests/attention_backward_oracle.py).  A `defect` argument restates a line the way a subtly
wrong kernel would compute it; the CPU part shows that the check rejects every one of them.
"""
import math

import numpy as np
import torch

from oracle import pointdsc_oracle as O
from oracle import sm_oracle
from pointdsc_amd import synthetic

F64 = torch.float64
FLOOR = 2e-6                 # SM eigenvector, confidences: the tolerance of the fixture tests of test_gpu_parity.py
FLOOR_RATIO = 1e-6           # eval row, the ratio columns: test_eval_stats_match_reference_losses
E32_MAX = 1e-3               # a case whose own fp32 evaluation is further than this from fp64 is ill-conditioned: not a test of a kernel


def bound(e32, floor=FLOOR):
    return max(4.0 * e32, floor)


def err(x, x64):
    """max|X - X64| / max|X64|"""
    return float((x.to(F64) - x64).abs().max() / x64.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# SM
# ---------------------------------------------------------------------------------------------------------------------------
def sigma2_f32(inlier_threshold):
    """The kernel's fp32 divisor: the threshold arrives as a float, sigma = thr / 3 and its square in double, then one rounding."""
    return float(np.float32((float(np.float32(inlier_threshold)) / 3.0) ** 2))


def _pair_dist(c):
    """[N,3] -> [N,N] Euclidean distances, axis by axis (an [N,N,3] difference tensor is 400 MB in fp64 at N = 4097)."""
    s = torch.zeros(c.shape[0], c.shape[0], dtype=c.dtype)
    for a in range(3):
        s += (c[:, None, a] - c[None, :, a]) ** 2
    return s ** 0.5


def sm_matrix64(corr, inlier_threshold, defect=None):
    """corr [N,6] -> M [N,N] fp64."""
    c = corr.to(F64)
    d = _pair_dist(c[:, 0:3]) - _pair_dist(c[:, 3:6])
    M = torch.clamp(4.5 - d ** 2 / 2 / sigma2_f32(inlier_threshold), min=0)
    if defect != "diagonal kept":
        M.fill_diagonal_(0)
    return M


def sm_power(M, iters, defect=None):
    """v = 1; iters x { v = M v; v /= |v| + 1e-6 } in the dtype of M (the lines of oracle/sm_oracle.py) -> v [N]."""
    n = M.shape[0]
    v = torch.ones(n, 1, dtype=M.dtype)
    last = v
    for _ in range(iters):
        last = v
        if defect == "ragged group dropped":               # the columns of the last, partial group of 4 never multiplied
            v = M[:, : n & ~3] @ v[: n & ~3]
        else:
            v = M @ v
        norm = torch.norm(v, dim=0, keepdim=True)
        if defect == "norm block missing":                 # one 16-row block's |y|^2 absent from the sum of the partials
            b0 = 16 if n > 16 else 0
            norm = (norm ** 2 - (v[b0:b0 + 16] ** 2).sum(dim=0, keepdim=True)).clamp(min=0) ** 0.5
        v = v / (norm + 1e-6)
    return (last if defect == "buffer parity" else v)[:, 0]


def sm_power64(M, iters):
    return sm_power(M.to(F64), iters)


def sm_order(v, defect=None):
    """Indices in descending order of v: NaN first (the largest, as torch.sort orders it), equal values by ascending index."""
    x = np.asarray(v.to(F64))
    nan = np.isnan(x)
    idx = np.arange(x.shape[0])
    tie = -idx if defect == "tie rule descending" else idx
    return np.lexsort((tie, -np.where(nan, 0.0, x), ~nan))


def sm_select(v, num_top, defect=None):
    """-> labels [N] fp32: 1 on the num_top first entries of sm_order."""
    labels = torch.zeros(v.shape[0], dtype=torch.float32)
    labels[torch.from_numpy(sm_order(v, defect)[:num_top].copy())] = 1
    return labels


def undecided(v64, num_top, tol):
    """Entries whose label a perturbation of `tol` per entry could change: kept entries within tol of the first dropped value, dropped
    entries within tol of the last kept one.  Empty when nothing or everything is kept."""
    n = v64.shape[0]
    if num_top <= 0 or num_top >= n:
        return torch.zeros(n, dtype=torch.bool)
    order = sm_order(v64)
    hi, lo = float(v64[order[num_top - 1]]), float(v64[order[num_top]])
    kept = sm_select(v64, num_top) > 0
    return (kept & (v64 <= lo + tol)) | (~kept & (v64 >= hi - tol))


def pose(src, tgt, weights, dtype):
    """O.rigid_transform_3d on [N,3] / [N] in `dtype` -> [4,4]."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return O.rigid_transform_3d(src[None].to(dtype), tgt[None].to(dtype), weights[None].to(dtype))[0]
    finally:
        torch.set_default_dtype(old)


# N: what it exercises (the matvec's 16-row block and the resident form's 20-row workgroup +- 1; the matrix kernel's 64-row tile and
# ld; one 256-column lane pass; the four-step unrolled trip with N % 4 = 3, 0, 1, 3; 257 partial sums)
SM_SIZES = (2, 5, 15, 16, 17, 20, 21, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 4097)
# regime -> make_pair arguments and the inlier threshold
SM_REGIMES = {"indoor": dict(inlier_ratio=0.3, scale=3.0, thr=0.10), "outdoor": dict(inlier_ratio=0.2, scale=60.0, thr=0.60)}
SM_TOP_RATIOS = (0.0, 0.1, 1.0)
SM_ALL_ZERO = (5, "indoor")        # seed 905: no two correspondences are compatible, M = 0
# (N, regime) -> seed, where seed 900 + N fails an input condition (test_sm_input_conditions names the condition)
SM_SEEDS = {(5, "outdoor"): 2905}


def sm_iters(n):
    return (1, 2, 10) if n <= 300 else (1, 10)


_SM = {}


def sm_case(n, regime):
    """The seeded pair of (N, regime) and, per iteration count, v64, the fp32 oracle's v32, e32 and the bound; computed once."""
    key = (n, regime)
    if key not in _SM:
        r = SM_REGIMES[regime]
        seed = SM_SEEDS.get(key, 900 + n)
        p = synthetic.make_pair(n, seed=seed, inlier_ratio=r["inlier_ratio"], scale=r["scale"], noise=r["scale"] / 300.0)
        corr, src, tgt = p["corr_pos"][0], p["src_keypts"][0], p["tgt_keypts"][0]
        M64, M32 = sm_matrix64(corr, r["thr"]), sm_oracle.sm_matrix(corr, r["thr"])
        case = dict(n=n, regime=regime, seed=seed, thr=r["thr"], corr=corr, src=src, tgt=tgt, M64=M64, v64={}, v32={}, e32={}, bound={})
        for it in sm_iters(n):
            v64, v32 = sm_power64(M64, it), sm_power(M32, it)
            e = err(v32, v64) if float(v64.abs().max()) > 0 else 0.0
            case["v64"][it], case["v32"][it], case["e32"][it], case["bound"][it] = v64, v32, e, bound(e)
        _SM[key] = case
    return _SM[key]


def sm_pose_reference(case, it, labels):
    """fp64 pose on v64 * labels, the fp32 oracle's pose on its own v32 * labels, the error scale and the floor of the pose check.
    Scale: the largest entry of the fp64 pose or coordinate.  Floor: the weights may be off by FLOOR max|v| each, which moves a
    weighted centroid by at most FLOOR * (num_top max w / sum w) of the coordinates' size -- first order, no rounding of the
    Procrustes itself counted."""
    w64 = case["v64"][it] * labels.to(F64)
    T64 = pose(case["src"], case["tgt"], w64, F64)
    T32 = pose(case["src"], case["tgt"], case["v32"][it] * labels, torch.float32)
    scale = max(float(T64.abs().max()), float(case["src"].abs().max()), float(case["tgt"].abs().max()))
    floor = FLOOR * float(labels.sum()) * float(w64.max()) / float(w64.sum())
    return T64, T32, scale, floor


def tie_case(n, equal):
    """Clusters of identical correspondences far apart: A on the odd indices; B on every even index (`equal`: |A| = |B|, everything
    ties) or on the even indices below n / 2, the other even ones isolated (|A| > |B|).  With one iteration the row sums are
    4.5 (|A| - 1), 4.5 (|B| - 1) and 0: exact in fp32.  -> corr [n,6] fp32."""
    corr = torch.zeros(n, 6)
    for i in range(0, n, 2):
        corr[i, 0] = 10.0 if equal or i < n // 2 else 100.0 * (i + 1)
    return corr


def nonfinite_case(kind):
    """N = 65, seed 965.  'nan': one coordinate of corr_pos is NaN; 'inf': one source coordinate is inf before the centring, so a
    whole column of corr_pos is -inf or NaN.  Either way every distance difference is NaN somewhere in every row.
    'inf entry': one coordinate of corr_pos alone is inf -- that correspondence is at distance inf from all others (M = 0 in its row
    and column) and at inf - inf = NaN from itself, which the zero diagonal overrides: everything stays finite, in the reference too."""
    p = synthetic.make_pair(65, seed=965, inlier_ratio=0.3, scale=3.0, noise=0.01)
    corr, src, tgt = p["corr_pos"][0].clone(), p["src_keypts"][0], p["tgt_keypts"][0]
    if kind == "nan":
        corr[33, 4] = float("nan")
    elif kind == "inf entry":
        corr[33, 0] = float("inf")
    else:
        both = torch.cat([src, tgt], dim=1)
        both[33, 0] = float("inf")
        corr = both - both.mean(dim=0, keepdim=True)
    return corr, src, tgt


# ---------------------------------------------------------------------------------------------------------------------------
# cal_confidence
# ---------------------------------------------------------------------------------------------------------------------------
CC_METHODS = ("eig_value", "eig_value_ratio", "xMx")
CC_SIZES = (1, 3, 4, 5, 16, 17, 255, 257, 1025)
CC_RATIO_ITERS = (0, 1, 10)
# (N, symmetric, |v|) whose ratio is not asserted: a symmetric M with unit v at N = 4 and 5 is the identity (no compatible pair), so
# B = I - v v^T annihilates the start vector 1 up to the 1e-6 of the normalisation: lambda2 along it is ~1e-5, the ratio ~5e5, and
# after a few steps round-off in the other directions (eigenvalue 1) decides the answer.  N = 1 has no ratio at all (B = 0).
CC_ILL = {(4, True, 1.0), (5, True, 1.0)}


def cal_confidence(M, v, method, iters, dtype=F64, defect=None):
    """M [N,N], v [N] -> the confidence as a python float: the reference's lines on a batch of one, in `dtype`."""
    M, leading_eig = M.to(dtype)[None], v.to(dtype)[None]
    if defect == "v normalised":
        leading_eig = leading_eig / torch.norm(leading_eig, dim=1, keepdim=True)
    if defect == "transposed":
        M = M.transpose(1, 2)
    max_eig_value = (leading_eig[:, None, :] @ M @ leading_eig[:, :, None]) / (leading_eig[:, None, :] @ leading_eig[:, :, None])
    if method == "eig_value":
        return float(max_eig_value)
    if method == "xMx":
        return float((leading_eig[:, None, :] @ M @ leading_eig[:, :, None]).squeeze(-1) / M.shape[1])
    B = M - max_eig_value * leading_eig[:, :, None] @ leading_eig[:, None, :]
    solution = torch.ones_like(B[:, :, 0:1])
    for _ in range(iters):
        solution = torch.bmm(B, solution)
        solution = solution / (torch.norm(solution, dim=1, keepdim=True) + 1e-6)
    second_eig = solution.squeeze(-1)
    second_eig_value = (second_eig[:, None, :] @ B @ second_eig[:, :, None]) / (second_eig[:, None, :] @ second_eig[:, :, None])
    return float(max_eig_value / second_eig_value)


def cal_confidence64(M, v, method, iters):
    return cal_confidence(M, v, method, iters, F64)


def cc_padded(M, v, pad):
    """The defect 'padding columns included': the sums run over ld = N + pad columns holding 1 -> (M', v') of size ld."""
    n = M.shape[0]
    Mp = torch.zeros(n + pad, n + pad, dtype=M.dtype)
    Mp[:n, :n] = M
    Mp[:n, n:] = 1.0
    return Mp, torch.cat([v, torch.ones(pad, dtype=v.dtype)])


_CC = {}


def cc_inputs(n, symmetric, vscale):
    """Seed 700 + N.  M = clamp(1 - d^2 / sigma^2, 0) of a synthetic pair (unit diagonal), times 0.5 + U(0,1) entrywise when not
    symmetric; v = the fp64 power-iteration vector of M (10 steps) cast to fp32, times vscale.  -> (M [N,N] fp32, v [N] fp32)."""
    key = (n, symmetric, vscale)
    if key not in _CC:
        p = synthetic.make_pair(max(n, 2), seed=700 + n, inlier_ratio=0.3, scale=3.0, noise=0.01)
        src, tgt = p["src_keypts"][0][:n], p["tgt_keypts"][0][:n]
        d = _pair_dist(src) - _pair_dist(tgt)
        M = torch.clamp(1.0 - d ** 2 / 0.1 ** 2, min=0)
        if not symmetric:
            M = M * (0.5 + torch.rand(n, n, generator=torch.Generator().manual_seed(700 + n)))
        v = (sm_power64(M, 10) * vscale).float()
        _CC[key] = (M.contiguous(), v)
    return _CC[key]


_CCREF = {}


def cc_reference(n, symmetric, vscale, method, iters):
    """-> (fp64 confidence, e32 of the fp32 yardstick), computed once per case."""
    key = (n, symmetric, vscale, method, iters)
    if key not in _CCREF:
        M, v = cc_inputs(n, symmetric, vscale)
        c64, c32 = cal_confidence64(M, v, method, iters), cal_confidence(M, v, method, iters, torch.float32)
        _CCREF[key] = (c64, abs(c32 - c64) / abs(c64) if c64 == c64 and c64 != 0 else float("inf"))
    return _CCREF[key]


def cc_cases():
    """(N, symmetric, vscale, method, iters) of every confidence asserted against fp64."""
    out = []
    for n in CC_SIZES:
        for symmetric in (True, False):
            for vscale in (1.0, 3.0):
                out += [(n, symmetric, vscale, "eig_value", 0), (n, symmetric, vscale, "xMx", 0)]
                if n > 1:
                    out += [(n, symmetric, vscale, "eig_value_ratio", it) for it in CC_RATIO_ITERS]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# eval row
# ---------------------------------------------------------------------------------------------------------------------------
def eval_row(trans, gt, pred, gt_labels, re_thre, te_thre, dtype=F64, defect=None):
    """trans, gt [bs,4,4]; pred, gt_labels [bs,N] -> [bs,9] fp64: libs/loss.py:44-51 and the stats row, evaluated in `dtype`."""
    rows = []
    thr_re, thr_te = float(np.float32(re_thre)), float(np.float32(te_thre))
    n = pred.shape[1]
    counted = n - n % 256 if defect == "label tail dropped" else n
    for i in range(trans.shape[0]):
        T, G = trans[i].to(dtype), gt[i].to(dtype)
        c = (torch.trace(T[:3, :3].T @ G[:3, :3]) - 1) / 2.0
        if defect == "nan swallowed":
            c = torch.nan_to_num(c, nan=-1.0)
        re = torch.acos(torch.clamp(c, min=-1, max=1)) * 180 / np.pi
        te = torch.sqrt(torch.sum((T[:3, 3] - G[:3, 3]) ** 2)) * 100
        if defect == "<=":
            success = bool(te <= thr_te) and bool(re <= thr_re)
        else:
            success = bool(te < thr_te) and bool(re < thr_re)
        p, g = pred[i, :counted] > 0, gt_labels[i, :counted] > 0
        gt_pos, pr_pos, tp = int(g.sum()), int(p.sum()), int((g & p).sum())
        one = torch.ones((), dtype=dtype)
        if defect == "precision nan":
            precision = float(tp * one / pr_pos) if pr_pos else float("nan")
        else:
            precision = float(tp * one / pr_pos) if pr_pos else 0.0
        recall = float(tp * one / gt_pos) if gt_pos else 0.0
        denom = 2 * tp + (pr_pos - tp) + (gt_pos - tp)
        f1 = float(2 * tp * one / denom) if denom else 0.0
        rows.append([float(success), float(re), float(te), float(gt_pos), float(gt_pos * one / n), float(tp), precision, recall, f1])
    return torch.tensor(rows, dtype=F64)


def eval_row64(trans, gt, pred, gt_labels, re_thre, te_thre):
    return eval_row(trans, gt, pred, gt_labels, re_thre, te_thre, F64)


def re_floor_deg(trans, gt):
    """One fp32 ulp of the trace carried through acos: 2^-23 * 3 / sqrt(max(1 - c^2, 2^-23)) radians, in degrees; [bs] fp64."""
    c = (((trans[:, :3, :3].to(F64) * gt[:, :3, :3].to(F64)).sum(dim=(1, 2)) - 1) / 2).clamp(-1, 1)
    return 2.0 ** -23 * 3 / torch.sqrt(torch.clamp(1 - c * c, min=2.0 ** -23)) * 180 / math.pi


TE_FLOOR_REL = 8 * 2.0 ** -24      # TE = sqrt(dx^2 + dy^2 + dz^2) * 100 in fp32: a difference, a square and two sums (5 roundings under
                                   # the root, halved by it), the root, the product: 4.5 x 2^-24; 8 x is the floor


def check_eval(got, ref64, yard, trans, gt, what=""):
    """Every column of `got` [bs,9] against the fp64 rows, with the fp32 yardstick rows `yard`; prints the worst figures; returns a
    list of failures (empty = the check passes) and the worst ratios per quantity."""
    got, fails, worst = got.to(F64), [], {}
    for col in (0, 3, 5):
        if not torch.equal(got[:, col], ref64[:, col]):
            fails.append(f"column {col} differs: {got[:, col].tolist()} vs {ref64[:, col].tolist()}")
    nan_ref = torch.isnan(ref64)
    if not torch.equal(torch.isnan(got), nan_ref):
        fails.append(f"NaN pattern differs: {torch.isnan(got).nonzero().tolist()} vs {nan_ref.nonzero().tolist()}")
    fin = ~nan_ref
    e = lambda x: torch.where(fin, (x - ref64).abs(), torch.zeros_like(ref64))
    eg, ey = e(torch.nan_to_num(got)), e(torch.nan_to_num(yard))
    b_re = torch.maximum(4 * ey[:, 1], torch.nan_to_num(re_floor_deg(trans, gt)))       # (a NaN row is judged by the NaN pattern above)
    b_te = torch.maximum(4 * ey[:, 2], TE_FLOOR_REL * torch.nan_to_num(ref64[:, 2]))
    b_ratio = torch.clamp(4 * ey[:, [4, 6, 7, 8]], min=FLOOR_RATIO)
    for name, dev, bnd, y in (("RE", eg[:, 1], b_re, ey[:, 1]), ("TE", eg[:, 2], b_te, ey[:, 2]),
                              ("ratios", eg[:, [4, 6, 7, 8]], b_ratio, ey[:, [4, 6, 7, 8]])):
        ratio = torch.where(bnd > 0, dev / torch.clamp(bnd, min=1e-300), torch.where(dev > 0, torch.full_like(dev, float("inf")), dev))
        worst[name] = float(ratio.max())
        print(f"eval {what} {name}: e32 {float(y.max()):.3e}  bound {float(bnd.max()):.3e}  device err {float(dev.max()):.3e}  "
              f"worst err / bound {worst[name]:.3f}")
        if worst[name] > 1.0:
            fails.append(f"{name}: err / bound {worst[name]:.3f}")
    return fails, worst


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def rotation_with_trace_above_3():
    """A seeded rotation in fp32 with every entry moved 4 ulps away from zero: the sum of squares of its entries is above 3 + 3 x 2^-22
    in exact arithmetic, so against itself its trace is above 3 in fp32 in any summation order (the worst accumulated rounding of nine
    terms is below 3 ulps of 3), and only the clamp keeps acos defined."""
    R = synthetic.random_rotation(np.random.RandomState(5)).astype(np.float32)
    for _ in range(4):
        R = np.nextafter(R, np.sign(R) * np.float32(np.inf), dtype=np.float32)
    assert float((R.astype(np.float64) ** 2).sum()) > 3 + 3 * 2.0 ** -22
    return R


POSE_ROWS = ("identity", "permutation", "same general", "1e-4 rad", "180 deg", "trace above 3", "RE below", "RE above", "TE below", "TE above",
             "NaN rotation", "NaN translation", "random 0", "random 1", "random 2", "random 3")
RE_THRE, TE_THRE = 15.0, 30.0


def pose_rows():
    """16 (pred, gt) poses, named by POSE_ROWS -> trans, gt [16,4,4] fp32."""
    rs = np.random.RandomState(77)
    G = synthetic.random_rotation(rs).astype(np.float64)
    g_t = np.array([0.3, -1.2, 2.0])
    perm = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
    above = rotation_with_trace_above_3().astype(np.float64)
    nan = float("nan")
    rows = {
        "identity": (_pose(np.eye(3), g_t), _pose(np.eye(3), g_t)),
        "permutation": (_pose(perm, g_t), _pose(perm, g_t)),
        "same general": (_pose(G, g_t), _pose(G, g_t)),
        "1e-4 rad": (_pose(_rot([1, 2, 3], 1e-4) @ G, g_t), _pose(G, g_t)),
        "180 deg": (_pose(_rot([0, 0, 1], math.pi) @ np.eye(3), g_t), _pose(np.eye(3), g_t)),
        "trace above 3": (_pose(above, g_t), _pose(above, g_t)),
        "RE below": (_pose(_rot([1, -1, 2], math.radians(RE_THRE - 0.01)) @ G, g_t), _pose(G, g_t)),
        "RE above": (_pose(_rot([1, -1, 2], math.radians(RE_THRE + 0.01)) @ G, g_t), _pose(G, g_t)),
        "TE below": (_pose(G, g_t + np.array([0.0, TE_THRE / 100 - 1e-4, 0.0])), _pose(G, g_t)),
        "TE above": (_pose(G, g_t + np.array([0.0, TE_THRE / 100 + 1e-4, 0.0])), _pose(G, g_t)),
        "NaN rotation": (_pose(G * np.array([[1, 1, 1], [1, nan, 1], [1, 1, 1]]), g_t), _pose(G, g_t)),
        "NaN translation": (_pose(G, g_t * np.array([1, nan, 1])), _pose(G, g_t)),
    }
    for i in range(4):
        rows[f"random {i}"] = (_pose(_rot(rs.randn(3), math.radians(rs.rand() * 40)) @ G, g_t + rs.randn(3) * 0.2), _pose(G, g_t))
    T = torch.from_numpy(np.stack([rows[k][0] for k in POSE_ROWS]).astype(np.float32))
    Gt = torch.from_numpy(np.stack([rows[k][1] for k in POSE_ROWS]).astype(np.float32))
    return T, Gt


LABEL_ROWS = ("random", "nothing predicted", "no ground truth", "both empty")
PRED_VALUES = (0.3, 7.0, -0.0, 0.0, float("nan"), -1.0)      # the first two count as predicted inliers, the others do not
EVAL_SIZES = (1, 63, 255, 256, 257, 1000, 70001)


def label_rows(n):
    """Four (pred, gt_labels) rows of length n, named by LABEL_ROWS; seed 500 + n.  Predictions are drawn from PRED_VALUES."""
    gen = torch.Generator().manual_seed(500 + n)
    pred = torch.tensor(PRED_VALUES)[torch.randint(0, len(PRED_VALUES), (4, n), generator=gen)]
    gtl = (torch.rand(4, n, generator=gen) < 0.4).float()
    neg = torch.tensor(PRED_VALUES[2:])[torch.randint(0, len(PRED_VALUES) - 2, (n,), generator=gen)]
    pred[1], pred[3] = neg, neg.flip(0)
    gtl[2], gtl[3] = 0.0, 0.0
    return pred, gtl
