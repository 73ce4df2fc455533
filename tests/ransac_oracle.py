"""fp64 numpy oracle of the correspondence-RANSAC contract (include/pointdsc_hip.h).

open3d is not available, so this transcription IS the contract; what it takes from open3d 0.9's
RegistrationRANSACBasedOnCorrespondence by recollection is a named rule:

DRAW_RULE      position j of iteration i of pair b uses the counter c = (b_global * I + i) * 8 + j;
               z = splitmix64(seed + (c + 1) * 0x9E3779B97F4A7C15) with the usual finaliser (^>>30, *0xBF58476D1CE4E5B9, ^>>27,
               *0x94D049BB133111EB, ^>>31); the position in L is (hi32(z) * M) >> 32.  With replacement.
               An explicit samples array replaces the draws; a position >= M or < 0 makes the hypothesis invalid.
hypothesis     Eigen's umeyama without scaling on the sample in fp64: means = sum * (1 / n), Sigma = (1 / n) sum (q - mB)(p - mA)^T,
               here through numpy.linalg.svd with the determinant correction (a FOREIGN solver: the library uses its Jacobi core).
               A non-finite pose is an invalid hypothesis: NaN pose, count 0, sumsq 0.
SCORE_RULE     over every l in L: d2 = |R src_l + t - tgt_l|^2 in fp64, inlier iff d2 < r * r; count = #inliers, sumsq = sum d2 over them.
SELECT_RULE    largest count, then smallest sumsq, then lowest iteration; a hypothesis with count 0 never wins.
NO_REFIT_RULE  the winner's pose is returned as solved from its sample.
Early outs     M < ransac_n, r <= 0 or r NaN: nothing wins (identity, zero labels, best_iter -1, fitness = rmse = 0).
"""
from __future__ import annotations

import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
SPLITMIX64_SEED0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC)   # the published vectors


def splitmix64(seed: int, c) -> np.ndarray:
    """The c-th output (c = 0, 1, ...) of splitmix64 seeded with `seed`: the finaliser of seed + (c + 1) * gamma, uint64 wrapping."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (np.asarray(c, dtype=np.uint64) + np.uint64(1)) * GAMMA
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draw_positions(seed: int, b_global: int, I: int, n: int, M: int) -> np.ndarray:
    """DRAW_RULE -> [I, n] int64 positions into L (all 0 when M == 0: nothing to draw from)."""
    with np.errstate(over="ignore"):
        i = np.arange(I, dtype=np.uint64)
        c = ((np.uint64(b_global) * np.uint64(I) + i) * np.uint64(8))[:, None] + np.arange(n, dtype=np.uint64)[None, :]
        hi = splitmix64(seed, c) >> np.uint64(32)
        return ((hi * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


def umeyama(P: np.ndarray, Q: np.ndarray):
    """Eigen::umeyama(P^T, Q^T, with_scaling = false) for a batch of samples: P, Q [I, n, 3] fp64 -> (T [I, 3, 4], singular values
    [I, 3]).  numpy.linalg.svd + the determinant correction."""
    n = P.shape[1]
    one_over_n = 1.0 / n
    mA = P.sum(axis=1) * one_over_n
    mB = Q.sum(axis=1) * one_over_n
    a = P - mA[:, None, :]
    b = Q - mB[:, None, :]
    sigma = np.einsum("inr,inc->irc", b, a) * one_over_n
    T = np.full((len(P), 3, 4), np.nan)
    sv = np.full((len(P), 3), np.nan)
    ok = np.isfinite(sigma).all(axis=(1, 2))
    if ok.any():
        U, S, Vt = np.linalg.svd(sigma[ok])
        d = np.ones((len(S), 3))
        d[:, 2] = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
        R = np.einsum("irk,ik,ikc->irc", U, d, Vt)
        T[ok, :, :3] = R
        T[ok, :, 3] = mB[ok] - np.einsum("irc,ic->ir", R, mA[ok])
        sv[ok] = S
    return T, sv


def score(T: np.ndarray, src_L: np.ndarray, tgt_L: np.ndarray, r: float):
    """SCORE_RULE for poses T [I, 3, 4] over the candidates -> (count [I] int64, sumsq [I], the smallest |d2 - r^2| / r^2)."""
    I = len(T)
    count = np.zeros(I, dtype=np.int64)
    sumsq = np.zeros(I)
    margin = np.inf
    if not (r > 0) or len(src_L) == 0:
        return count, sumsq, margin
    r2 = r * r
    x, y, z = (src_L[:, k].astype(np.float64)[None, :] for k in range(3))
    with np.errstate(invalid="ignore"):
        d2 = np.zeros((I, len(src_L)))
        for k in range(3):
            dk = T[:, k, 0, None] * x + T[:, k, 1, None] * y + T[:, k, 2, None] * z + T[:, k, 3, None] - tgt_L[:, k].astype(np.float64)[None, :]
            d2 += dk * dk
        inl = d2 < r2
    fin = np.isfinite(d2)
    if fin.any():
        margin = float(np.abs(d2[fin] - r2).min() / r2)
    return inl.sum(axis=1), np.where(inl, d2, 0.0).sum(axis=1), margin


def select(count: np.ndarray, sumsq: np.ndarray) -> int:
    """SELECT_RULE -> the winning iteration, -1 if no hypothesis has an inlier."""
    cand = np.flatnonzero(np.asarray(count) > 0)
    if len(cand) == 0:
        return -1
    order = np.lexsort((cand, np.asarray(sumsq)[cand], -np.asarray(count, dtype=np.int64)[cand]))
    return int(cand[order[0]])


def candidates(mask, N: int) -> np.ndarray:
    return np.arange(N) if mask is None else np.flatnonzero(np.asarray(mask) > 0)


def outputs(src, tgt, L, r, best: int, best_pose, best_count: int, best_sumsq: float):
    """trans / labels / fitness / inlier_rmse of a winner (or of nothing) as the contract defines them."""
    N = len(src)
    trans = np.eye(4, dtype=np.float32)
    labels = np.zeros(N, dtype=np.float32)
    if best < 0:
        return trans, labels, 0.0, 0.0
    trans[:3, :] = best_pose.astype(np.float32)
    x = src[L].astype(np.float64)
    q = tgt[L].astype(np.float64)
    d2 = np.zeros(len(L))
    with np.errstate(invalid="ignore"):
        for k in range(3):
            dk = best_pose[k, 0] * x[:, 0] + best_pose[k, 1] * x[:, 1] + best_pose[k, 2] * x[:, 2] + best_pose[k, 3] - q[:, k]
            d2 += dk * dk
        labels[L[d2 < r * r]] = 1.0
    return trans, labels, best_count / len(L), float(np.sqrt(best_sumsq / best_count))


def ransac(src, tgt, r: float, ransac_n: int, I: int, seed: int = 0, b_global: int = 0, mask=None, samples=None) -> dict:
    """The whole contract for one pair: src, tgt [N, 3] fp32."""
    src = np.asarray(src, dtype=np.float32)
    tgt = np.asarray(tgt, dtype=np.float32)
    N = len(src)
    L = candidates(mask, N)
    M = len(L)
    pos = draw_positions(seed, b_global, I, ransac_n, M) if samples is None else np.asarray(samples, dtype=np.int64)
    enabled = M >= ransac_n and r > 0
    valid = np.full(I, bool(enabled)) & ((pos >= 0) & (pos < M)).all(axis=1)
    T = np.full((I, 3, 4), np.nan)
    sv = np.full((I, 3), np.nan)
    if valid.any():
        idx = L[pos[valid]]
        T[valid], sv[valid] = umeyama(src[idx].astype(np.float64), tgt[idx].astype(np.float64))
    valid &= np.isfinite(T).all(axis=(1, 2))
    T[~valid] = np.nan
    count, sumsq, margin = score(T, src[L], tgt[L], r if enabled else 0.0)
    best = select(count, sumsq)
    trans, labels, fitness, rmse = outputs(src, tgt, L, r, best, T[best] if best >= 0 else None, int(count[best]) if best >= 0 else 0,
                                           float(sumsq[best]) if best >= 0 else 0.0)
    distinct = np.array([len(set(row)) == ransac_n for row in pos])
    return {"L": L, "M": M, "samples": pos, "valid": valid, "distinct": distinct, "hyp_trans": T, "sv": sv, "hyp_count": count,
            "hyp_sumsq": sumsq, "margin": margin, "best_iter": best, "trans": trans, "labels": labels, "fitness": fitness,
            "inlier_rmse": rmse}


def pose_errors(trans: np.ndarray, gt: np.ndarray):
    """(rotation error [deg], translation error [cm]) as the evaluation measures them."""
    R = np.asarray(trans, dtype=np.float64)[:3, :3]
    G = np.asarray(gt, dtype=np.float64)
    c = np.clip((np.trace(R.T @ G[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(np.asarray(trans, dtype=np.float64)[:3, 3] - G[:3, 3]) * 100.0)
