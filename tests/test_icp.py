"""f-5: the evaluation's ICP post-step (pointdsc_amd.icp, csrc/icp.hip) against an fp64 numpy restatement of open3d 0.9's
point-to-point registration_icp (evaluation/benchmark_utils.py:40-56; the algorithm is written out in DESIGN.md section 8 f-5).

open3d is not available, so the oracle below IS the contract: it follows RegistrationICP / GetRegistrationResultAndCorrespondences /
TransformationEstimationPointToPoint (Eigen::umeyama) step by step.  Two details of open3d cannot be checked here and are named
rules: the squared radius is rounded to fp32 and compared with a strict '<' (FLANN_RADIUS_RULE), and among distinct targets at
exactly equal distance the lowest target index wins (TIE_RULE).  The oracle also records the smallest margin of every discrete
decision, so that a pair that sits on a near-tie is reported and compared by its final pose only.
"""
from __future__ import annotations

import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"

FLANN_RADIUS_RULE = "d2 < float32(r * r)"      # fp64 squared distance against the fp32-rounded squared radius, strict
TIE_RULE = "lowest target index"               # among distinct targets at exactly equal distance
NEAR_TIE = 1e-9                                # relative margin below which a decision counts as a near-tie
IDENTITY_PREC = 1e-12                          # Eigen isIdentity() default precision (open3d skips an identity init)

try:
    from scipy.spatial import cKDTree as _KDTree
except ImportError:  # pragma: no cover - brute force below
    _KDTree = None


# ---------------------------------------------------------------------------------------------------------------------------
# oracle (fp64 numpy)
# ---------------------------------------------------------------------------------------------------------------------------
def _apply(T, P):
    """Eigen (T * (x, y, z, 1)).head<3>() / w, written out in the kernel's order."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    w = T[3, 0] * x + T[3, 1] * y + T[3, 2] * z + T[3, 3]
    return np.stack([(T[i, 0] * x + T[i, 1] * y + T[i, 2] * z + T[i, 3]) / w for i in range(3)], axis=1)


def _candidates(P, Q, r):
    """(row, col) of every (source, target) pair within r (1 + 1e-3): a superset of everything the radius test can accept."""
    rr = r * (1.0 + 1e-3)
    if _KDTree is not None:
        lists = _KDTree(Q).query_ball_point(P, rr)
        lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
        rows = np.repeat(np.arange(len(P)), lens)
        cols = np.fromiter((j for x in lists for j in x), dtype=np.int64, count=int(lens.sum()))
        return rows, cols
    rows, cols = [], []
    for s in range(0, len(P), 256):
        d2 = ((P[s:s + 256, None, :] - Q[None, :, :]) ** 2).sum(-1)
        r_, c_ = np.nonzero(d2 < rr * rr)
        rows.append(r_ + s)
        cols.append(c_)
    return np.concatenate(rows), np.concatenate(cols)


def _evaluate(P, Q, r2, r):
    """GetRegistrationResultAndCorrespondences: nearest target within the radius per source point (TIE_RULE), fitness, rmse,
    and the smallest relative margin of the radius test / nearest-versus-second-nearest decision."""
    n = len(P)
    corr = np.full(n, -1, dtype=np.int64)
    d2best = np.zeros(n)
    margin = math.inf
    if len(Q) and n:
        rows, cols = _candidates(P, Q, r)
        if len(rows):
            d = P[rows] - Q[cols]
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            margin = min(margin, float(np.abs(d2 - r2).min() / r2))
            ok = d2 < r2
            rows, cols, d2 = rows[ok], cols[ok], d2[ok]
        if len(rows):
            order = np.lexsort((cols, d2, rows))
            rows, cols, d2 = rows[order], cols[order], d2[order]
            first = np.r_[True, rows[1:] != rows[:-1]]
            corr[rows[first]] = cols[first]
            d2best[rows[first]] = d2[first]
            # second nearest among targets at other coordinates (duplicates of the winner do not change the result)
            other = np.any(Q[cols] != Q[corr[rows]], axis=1)
            if other.any():
                gap = d2[other] - d2best[rows[other]]
                margin = min(margin, float(gap.min() / r2))
    sel = corr >= 0
    k = int(sel.sum())
    fitness = k / n if k else 0.0
    rmse = math.sqrt(d2best[sel].sum() / k) if k else 0.0
    return corr, fitness, rmse, margin


def _umeyama(A, B):
    """Eigen::umeyama(A^T, B^T, false): the rigid motion of the rows of A onto the rows of B."""
    n = len(A)
    one_over_n = 1.0 / n
    mA, mB = A.sum(0) * one_over_n, B.sum(0) * one_over_n
    sigma = (B - mB).T @ (A - mA) * one_over_n
    U, _, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = mB - T[:3, :3] @ mA
    return T


def _is_identity(T):
    d = np.abs(T - np.eye(4))
    diag = np.abs(np.diag(T))
    return bool(np.all(d[~np.eye(4, dtype=bool)] <= IDENTITY_PREC) and
                np.all(np.abs(np.diag(T) - 1.0) <= IDENTITY_PREC * np.minimum(diag, 1.0)))


def icp_oracle(S, Q, init, r=0.10, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """open3d 0.9 RegistrationICP with TransformationEstimationPointToPoint, fp64.  S [Ns,3], Q [Nt,3] fp32; init [4,4] fp32."""
    S = np.asarray(S, np.float32).astype(np.float64)
    Q = np.asarray(Q, np.float32).astype(np.float64)
    T = np.asarray(init, np.float32).astype(np.float64)
    if not r > 0:
        return {"T": T, "fitness": 0.0, "rmse": 0.0, "corr": np.full(len(S), -1), "iterations": 0, "margin": math.inf}
    r2 = float(np.float32(r * r))                       # FLANN_RADIUS_RULE
    P = S.copy() if _is_identity(T) else _apply(T, S)
    corr, fit, rmse, margin = _evaluate(P, Q, r2, r)
    it = 0
    while it < max_iteration:
        sel = corr >= 0
        U = _umeyama(P[sel], Q[corr[sel]]) if sel.any() else np.eye(4)
        T = U @ T
        P = _apply(U, P)
        prev_fit, prev_rmse = fit, rmse
        corr, fit, rmse, m = _evaluate(P, Q, r2, r)
        margin = min(margin, m)
        it += 1
        df, dr = abs(prev_fit - fit), abs(prev_rmse - rmse)
        margin = min(margin, abs(df - relative_fitness) / relative_fitness, abs(dr - relative_rmse) / relative_rmse)
        if df < relative_fitness and dr < relative_rmse:
            break
    return {"T": T, "fitness": fit, "rmse": rmse, "corr": corr, "iterations": it, "margin": margin}


def _rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tests: the oracle itself, the ABI, argument checks
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_recovers_rigid_motion_from_exact_copy():
    rs = np.random.RandomState(3)
    S = rs.uniform(-1, 1, (400, 3)).astype(np.float32)
    G = np.eye(4)
    G[:3, :3] = _rot([1, 2, 3], 3.0)
    G[:3, 3] = [0.02, -0.03, 0.01]
    Q = _apply(G, S.astype(np.float64)).astype(np.float32)
    res = icp_oracle(S, Q, np.eye(4, dtype=np.float32))
    assert res["fitness"] == 1.0
    assert np.abs(res["T"] - G).max() < 1e-6
    assert res["rmse"] < 1e-6


def test_oracle_returns_init_when_nothing_within_radius():
    rs = np.random.RandomState(4)
    S = rs.uniform(0, 1, (50, 3)).astype(np.float32)
    Q = (S + 10.0).astype(np.float32)
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = [0.5, 0, 0]
    res = icp_oracle(S, Q, init)
    assert res["iterations"] == 1 and res["fitness"] == 0.0 and res["rmse"] == 0.0
    np.testing.assert_array_equal(res["T"], init.astype(np.float64))


def _three_squares(m):
    """Integers (a, b, c) with a^2 + b^2 + c^2 == m."""
    for a in range(int(math.isqrt(m)), -1, -1):
        b = np.arange(0, int(math.isqrt(m - a * a)) + 1, dtype=np.int64)
        c2 = m - a * a - b * b
        c = np.round(np.sqrt(c2)).astype(np.int64)
        hit = np.flatnonzero(c * c == c2)
        if len(hit):
            return a, int(b[hit[0]]), int(c[hit[0]])
    raise AssertionError(m)


def test_oracle_fitness_rmse_definitions_on_four_points():
    r = 0.10
    r2 = float(np.float32(r * r))                       # 0.00999999977648258 = m 2^-30
    m = int(r2 * 2.0 ** 30)
    assert m * 2.0 ** -30 == r2
    a, b, c = _three_squares(m)
    on = np.array([a, b, c], np.float64) * 2.0 ** -15     # fp32-exact offset whose fp64 squared length is exactly r2
    assert on[0] ** 2 + on[1] ** 2 + on[2] ** 2 == r2
    S = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float32)
    Q = np.array([[0, 0.03, 0], [1, 0.05, 0], [2 + on[0], on[1], on[2]], [3, 0.5, 0]], np.float32)
    Qd = Q.astype(np.float64)
    assert np.array_equal(Qd[2] - [2, 0, 0], on)
    P = S.astype(np.float64)
    corr, fit, rmse, margin = _evaluate(P, Qd, r2, r)
    # exactly on the fp32-rounded squared radius: excluded by the strict '<', and reported as a zero-margin decision
    assert list(corr) == [0, 1, -1, -1] and margin == 0.0
    assert fit == 2 / 4
    assert rmse == pytest.approx(math.sqrt((Qd[0, 1] ** 2 + Qd[1, 1] ** 2) / 2), rel=1e-15)
    # one unit of 2^-15 closer along the largest axis: accepted
    Q2 = Q.copy()
    k = int(np.argmax([a, b, c]))
    Q2[2, k] = np.float32(Qd[2, k] - 2.0 ** -15 * np.sign(Qd[2, k] - S[2, k]))
    corr2, fit2, _, _ = _evaluate(P, Q2.astype(np.float64), r2, r)
    assert corr2[2] == 2 and fit2 == 0.75
    # the fp64 radius 0.1 itself would have accepted the point on the rounded radius (r2 < 0.1^2 in fp64)
    assert r2 < r * r


def test_oracle_tie_rule_lowest_index():
    S = np.zeros((1, 3))
    Q = np.array([[0.05, 0, 0], [-0.05, 0, 0], [0, 0.05, 0]])
    corr, _, _, margin = _evaluate(S, Q, float(np.float32(0.01)), 0.1)
    assert corr[0] == 0 and margin == 0.0


def test_header_declares_icp_and_library_exports_it():
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    assert re.search(r"\bsize_t\s+pdsc_icp_workspace_bytes\s*\(", header)
    assert re.search(r"\bint\s+pdsc_icp_refine\s*\(", header)
    from pointdsc_amd import _lib
    assert "pdsc_icp_refine" in _lib.SIGNATURES and "pdsc_icp_workspace_bytes" in _lib.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ("pdsc_icp_refine", "pdsc_icp_workspace_bytes"):
        assert re.search(rf"\bT {name}\b", out), name
    lib = _lib.load()
    assert lib.pdsc_icp_workspace_bytes(2, 5000, 4000) >= 2 * (5000 * 28 + 4000 * 16)
    assert lib.pdsc_icp_workspace_bytes(0, 10, 10) == 0
    # argument validation happens before any HIP call
    assert lib.pdsc_icp_refine(None, None, None, None, None, 0.1, 1e-6, 1e-6, 30, None, None, None, None, None, None, None, 0,
                               1, 10, 10, None) == -1
    assert b"null pointer" in lib.pdsc_last_error()
    p = C.c_void_p(16)
    assert lib.pdsc_icp_refine(p, p, p, None, None, 0.1, 1e-6, 1e-6, 30, p, None, p, p, p, p, p, 0, 1, 10, 10, None) == -1
    assert b"workspace" in lib.pdsc_last_error()


def test_icp_argument_checks_on_cpu():
    from pointdsc_amd import icp_refine, registration_icp
    src = torch.zeros(1, 10, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        icp_refine(src, src, torch.eye(4)[None])
    with pytest.raises(ValueError, match=r"\[bs,N,3\]"):
        icp_refine(torch.zeros(1, 10, 2), src, torch.eye(4)[None])
    with pytest.raises(ValueError):
        icp_refine(torch.zeros(10, 3), src, torch.eye(4)[None])
    with pytest.raises(ValueError):
        icp_refine([torch.zeros(0, 3)], [torch.zeros(5, 3)], torch.eye(4)[None])
    with pytest.raises(ValueError, match="NaN"):
        registration_icp(src, src, torch.eye(4)[None], max_correspondence_distance=float("nan"))
    with pytest.raises(ValueError, match="max_iteration"):
        registration_icp(src, src, torch.eye(4)[None], max_iteration=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def _gpu_run(S_list, Q_list, inits, **kw):
    from pointdsc_amd import registration_icp
    dev = torch.device("cuda:0")
    res = registration_icp([torch.from_numpy(np.ascontiguousarray(s, np.float32)).to(dev) for s in S_list],
                           [torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev) for q in Q_list],
                           torch.from_numpy(np.ascontiguousarray(np.stack(inits), np.float32)).to(dev), **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def _compare(name, S, Q, init, got, b, **kw):
    """One pair of a GPU result against the oracle (see the module docstring for the near-tie rule)."""
    ref = icp_oracle(S, Q, init, **kw)
    T32 = got["transformation"][b]
    if ref["margin"] < NEAR_TIE:
        print(f"[icp] {name}: near-tie (oracle margin {ref['margin']:.2e}): final pose only")
        assert np.abs(T32 - ref["T"]).max() < 1e-4, name
        return ref
    assert int(got["iterations"][b]) == ref["iterations"], (name, int(got["iterations"][b]), ref["iterations"])
    assert int(got["num_correspondences"][b]) == int((ref["corr"] >= 0).sum()), name
    assert float(got["fitness"][b]) == ref["fitness"], name
    assert abs(float(got["inlier_rmse"][b]) - ref["rmse"]) <= 1e-9 * max(ref["rmse"], 1e-300), name
    assert np.abs(T32 - ref["T"]).max() < 1e-6, (name, np.abs(T32 - ref["T"]).max())
    # the correspondence set: the oracle's final set equals the set of the device's final pose (margins >= 1e-9 above)
    P = _apply(got["transformation_f64"][b], np.asarray(S, np.float32).astype(np.float64))
    corr, _, _, _ = _evaluate(P, np.asarray(Q, np.float32).astype(np.float64), float(np.float32(kw.get("r", 0.1) ** 2)),
                              kw.get("r", 0.1))
    np.testing.assert_array_equal(corr, ref["corr"], err_msg=name)
    print(f"[icp] {name}: iterations {ref['iterations']} corr {int((ref['corr'] >= 0).sum())} fitness {ref['fitness']:.6f} "
          f"rmse {ref['rmse']:.6e} max|dT| {np.abs(T32 - ref['T']).max():.2e} margin {ref['margin']:.2e}")
    return ref


def _perturbed(G, deg, cm, seed):
    rs = np.random.RandomState(seed)
    T = np.asarray(G, np.float64).copy()
    D = np.eye(4)
    D[:3, :3] = _rot(rs.standard_normal(3), deg)
    d = rs.standard_normal(3)
    D[:3, 3] = d / np.linalg.norm(d) * cm / 100.0
    return (D @ T).astype(np.float32)


def _demo_case(seed=0):
    from pointdsc_amd import harness
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    tgt, G, _ = harness.second_view(cloud, seed)
    return cloud, tgt, _perturbed(G, 2.0, 5.0, 100 + seed), G


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1000_s1", "n5000_s5", "kitti_n1500_s4", "lomatch_n10000_s7"])
def test_icp_matches_oracle_on_reference_fixtures(name):
    d = np.load(GOLDEN / f"{name}.npz")
    S, Q, init = d["src_keypts"][0], d["tgt_keypts"][0], d["ref_final_trans"][0]
    got = _gpu_run([S], [Q], [init])
    _compare(name, S, Q, init, got, 0)


@pytest.mark.gpu
def test_icp_matches_oracle_on_demo_cloud_second_view():
    S, Q, init, G = _demo_case(0)
    assert len(S) != len(Q)
    got = _gpu_run([S], [Q], [init])
    ref = _compare("demo second_view", S, Q, init, got, 0)
    # ICP from a 2 deg / 5 cm perturbation moves the pose towards the ground truth
    from oracle import pointdsc_oracle as O
    re0, te0 = O.registration_errors(torch.from_numpy(init), torch.from_numpy(G))
    re1, te1 = O.registration_errors(torch.from_numpy(got["transformation"][0]), torch.from_numpy(G))
    assert re1 < re0 and te1 < te0, (re0, te0, re1, te1)
    assert ref["iterations"] >= 2


@pytest.mark.gpu
def test_icp_degenerate_correspondence_sets():
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = [0.01, -0.02, 0.005]
    # 1 correspondence: the update is the exact translation onto the target
    S1 = np.array([[0.3, 0.2, 0.1], [5, 5, 5]], np.float32)
    Q1 = np.array([[0.32, 0.17, 0.12], [-5, -5, -5]], np.float32)
    # 2 correspondences of a rigid copy: only the two endpoints are determined
    S2 = np.array([[0, 0, 0], [0.05, 0.02, 0.0]], np.float32)
    G = np.eye(4)
    G[:3, :3] = _rot([0, 0, 1], 10)
    G[:3, 3] = [0.01, 0.01, 0]
    Q2 = _apply(G, S2.astype(np.float64)).astype(np.float32)
    # empty set: init comes back
    S3 = np.array([[0, 0, 0]], np.float32)
    Q3 = np.array([[1, 1, 1]], np.float32)
    got = _gpu_run([S1, S2, S3], [Q1, Q2, Q3], [init, init, init])
    T1 = got["transformation_f64"][0]
    assert got["num_correspondences"][0] == 1
    np.testing.assert_allclose(_apply(T1, S1[:1].astype(np.float64)), Q1[:1].astype(np.float64), atol=1e-12)
    np.testing.assert_allclose(T1[:3, :3], np.eye(3), atol=1e-12)
    assert got["num_correspondences"][1] == 2
    mapped = _apply(got["transformation_f64"][1], S2.astype(np.float64))
    assert np.abs(mapped - Q2.astype(np.float64)).max() < 1e-6
    assert got["num_correspondences"][2] == 0 and got["iterations"][2] == 1 and got["fitness"][2] == 0.0
    np.testing.assert_array_equal(got["transformation"][2], init)


@pytest.mark.gpu
def test_icp_non_finite_init_or_point_gives_nan_pose():
    S, Q, init, _ = _demo_case(1)
    bad_init = init.copy()
    bad_init[0, 3] = np.nan
    S_bad = S.copy()
    S_bad[17, 1] = np.inf
    got = _gpu_run([S, S_bad, S], [Q, Q, Q], [bad_init, init, init])
    for b in (0, 1):
        assert np.isnan(got["transformation"][b]).all() and got["iterations"][b] == 0
    assert np.isfinite(got["transformation"][2]).all() and got["iterations"][2] > 0


@pytest.mark.gpu
def test_icp_max_distance_not_positive_returns_init():
    S, Q, init, _ = _demo_case(2)
    got = _gpu_run([S], [Q], [init], max_correspondence_distance=0.0)
    np.testing.assert_array_equal(got["transformation"][0], init)
    assert got["iterations"][0] == 0 and got["fitness"][0] == 0.0


@pytest.mark.gpu
def test_icp_duplicate_targets_equal_deduplicated():
    S, Q, init, _ = _demo_case(3)
    rs = np.random.RandomState(5)
    dup = np.concatenate([Q, Q[rs.randint(0, len(Q), 2000)]])
    perm = rs.permutation(len(dup))
    Qd = dup[perm]
    # de-duplicated in first-occurrence order of the permuted set
    _, first = np.unique(Qd, axis=0, return_index=True)
    Qu = Qd[np.sort(first)]
    got = _gpu_run([S, S], [Qd, Qu], [init, init])
    for k in ("transformation_f64", "fitness", "inlier_rmse", "num_correspondences", "iterations"):
        np.testing.assert_array_equal(got[k][0], got[k][1], err_msg=k)


@pytest.mark.gpu
def test_icp_ragged_batch_is_bitwise_each_pair_alone():
    cases = [_demo_case(s) for s in range(4)]
    d = np.load(GOLDEN / "n1000_s1.npz")
    S_list = [c[0] for c in cases] + [d["src_keypts"][0], cases[0][0][:700]]
    Q_list = [c[1] for c in cases] + [d["tgt_keypts"][0], cases[0][1][:2500]]
    inits = [c[2] for c in cases] + [d["ref_final_trans"][0], cases[0][2]]
    assert len({len(s) for s in S_list}) > 1 and any(len(s) != len(q) for s, q in zip(S_list, Q_list))
    batch = _gpu_run(S_list, Q_list, inits)
    for b in range(len(S_list)):
        alone = _gpu_run([S_list[b]], [Q_list[b]], [inits[b]])
        for k in ("transformation", "transformation_f64", "fitness", "inlier_rmse", "num_correspondences", "iterations"):
            np.testing.assert_array_equal(batch[k][b], alone[k][0], err_msg=f"pair {b} {k}")


@pytest.mark.gpu
def test_icp_32_pairs_repeatable_and_graph_capturable():
    from pointdsc_amd import registration_icp
    d = np.load(GOLDEN / "n5000_s5.npz")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(9)
    S = torch.from_numpy(np.repeat(d["src_keypts"], 32, 0)).to(dev)
    Q = torch.from_numpy(np.repeat(d["tgt_keypts"], 32, 0)).to(dev)
    init = torch.from_numpy(np.stack([_perturbed(d["ref_final_trans"][0], 1.0, 2.0, int(s)) for s in rs.randint(0, 10**6, 32)])).to(dev)
    a = registration_icp(S, Q, init)
    b = registration_icp(S, Q, init)
    torch.cuda.synchronize()
    for k in ("transformation", "transformation_f64", "fitness", "inlier_rmse", "num_correspondences", "iterations"):
        assert torch.equal(a[k], b[k]), k
    # graph capture: one launch, no host synchronisation inside the call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        registration_icp(S, Q, init)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = registration_icp(S, Q, init)
    g.replay()
    torch.cuda.synchronize()
    for k in ("transformation", "transformation_f64", "fitness", "inlier_rmse", "num_correspondences", "iterations"):
        assert torch.equal(a[k], c[k]), k
    c["transformation"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a["transformation"], c["transformation"])


@pytest.mark.gpu
def test_eval_scene_use_icp_refines_the_pose():
    from pointdsc_amd import PointDSC, harness, workloads
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    kw = dict(workloads.BASE_MODEL)
    model = PointDSC(**kw)
    model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    model = model.eval().cuda()
    pairs = list(harness.demo_pairs(cloud, 3))
    base = harness.eval_scene(model, pairs, inlier_threshold=kw["inlier_threshold"], batch_size=3)
    refined = harness.eval_scene(model, pairs, inlier_threshold=kw["inlier_threshold"], batch_size=3, use_icp=True)
    assert refined.shape == base.shape == (3, 12)
    # label columns come from the forward and stay; the pose columns come from the refined pose
    np.testing.assert_array_equal(refined[:, 3:9], base[:, 3:9])
    assert not np.array_equal(refined[:, 1:3], base[:, 1:3])
    assert refined[:, 1].mean() <= base[:, 1].mean() and refined[:, 2].mean() <= base[:, 2].mean(), (base[:, 1:3], refined[:, 1:3])
