"""f-8: pose-graph optimisation on the device (pointdsc_amd.multiway.global_optimization / pose_graph_nodes; csrc/posegraph.hip)
against an fp64 numpy restatement of open3d 0.9's GlobalOptimization with GlobalOptimizationLevenbergMarquardt and default
criteria, as multiway/test_multi_ate.py:166-174 calls it.

open3d is not available, so the oracle below IS the contract (the same text is in
include/pointdsc_hip.h).  Two details that cannot be checked against open3d are named rules:
  INVERSE_RULE  the inverse of a pose is [R^-1, -R^-1 t] with R^-1 = adj(R) / det(R), not R^T;
  SOLVE_RULE    open3d solves with Eigen's ldlt(); any backward-stable factorisation of H + lambda I satisfies the contract within
                the tolerance below.
Besides its results the oracle returns the smallest margin of every discrete decision of a run (|rho| of each trial, the relative
gap of each stop criterion it evaluated, |confidence - threshold| at each pruning): every test graph has all margins >= MIN_MARGIN,
checked when the seeds were chosen and asserted here, so that the device must take the same decisions.

Tolerance on poses and confidences: the oracle runs with two solve arms (numpy.linalg.solve and scipy's Cholesky); the largest
difference of their final pose entries and confidences is a graph's floor, and the device is allowed 100 x that floor (it differs
from both arms in summation order and in its fused multiply-adds).  Floors and observed maxima are printed before asserting.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"

MIN_MARGIN = 1e-6
EDGE_DISTANCE = 0.05 * 1.4
OPTIONS = dict(max_correspondence_distance=EDGE_DISTANCE, edge_prune_threshold=0.25, preference_loop_closure=20.0, reference_node=0)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle (fp64 numpy)
# ---------------------------------------------------------------------------------------------------------------------------
def _generators():
    G = np.zeros((6, 4, 4))
    G[0][1, 2], G[0][2, 1] = -1, 1
    G[1][0, 2], G[1][2, 0] = 1, -1
    G[2][0, 1], G[2][1, 0] = -1, 1
    G[3][0, 3] = G[4][1, 3] = G[5][2, 3] = 1
    return G


GEN = _generators()


def inverse_rule(T):
    """INVERSE_RULE: [R^-1, -R^-1 t; 0 0 0 1] with R^-1 = adj(R) / det(R)."""
    (a, b, c), (d, e, f), (g, h, i) = T[0, :3], T[1, :3], T[2, :3]
    c00, c10, c20 = e * i - f * h, f * g - d * i, d * h - e * g
    det = (a * c00 + b * c10) + c * c20
    Ri = np.array([[c00, c * h - b * i, b * f - c * e], [c10, a * i - c * g, c * d - a * f], [c20, b * g - a * h, a * e - b * d]]) / det
    O = np.eye(4)
    O[:3, :3] = Ri
    O[:3, 3] = -((Ri[:, 0] * T[0, 3] + Ri[:, 1] * T[1, 3]) + Ri[:, 2] * T[2, 3])
    return O


def lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def vec2mat(v):
    sx, cx, sy, cy, sz, cz = math.sin(v[0]), math.cos(v[0]), math.sin(v[1]), math.cos(v[1]), math.sin(v[2]), math.cos(v[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = v[3:6]
    return T


def mat2vec(T, margins=None):
    sy = math.hypot(T[0, 0], T[1, 0])
    if margins is not None:
        margins["stop"].append(abs(sy - 1e-6) / max(sy, 1e-6))
    if not sy < 1e-6:
        return np.array([math.atan2(T[2, 1], T[2, 2]), math.atan2(-T[2, 0], sy), math.atan2(T[1, 0], T[0, 0]), T[0, 3], T[1, 3], T[2, 3]])
    return np.array([math.atan2(-T[1, 2], T[1, 1]), math.atan2(-T[2, 0], sy), 0.0, T[0, 3], T[1, 3], T[2, 3]])


def _solve_numpy(A, b):
    return np.linalg.solve(A, b)


def _solve_cholesky(A, b):
    import scipy.linalg
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), b)


SOLVERS = {"numpy": _solve_numpy, "cholesky": _solve_cholesky}


def _less(a, thr, margins):
    """a < thr, with the relative gap of the comparison noted."""
    margins["stop"].append(abs(a - thr) / max(abs(a), abs(thr), 1e-300))
    return a < thr


class _Pass:
    """One optimisation pass over the live edges (steps 1-11 of the contract)."""

    def __init__(self, edges, live, opts, solve, margins):
        self.src, self.tgt, self.X, self.Lam, self.unc = edges
        self.live, self.opts, self.solve, self.margins = live, opts, solve, margins
        self.Xi = [inverse_rule(x) for x in self.X]
        idx = np.flatnonzero(live)
        self.idx = idx
        d = opts["max_correspondence_distance"]
        self.w = (opts["preference_loop_closure"] * (d * d)) * (self.Lam[idx, 5, 5].sum() / len(idx)) if len(idx) else 0.0

    def residuals(self, poses, jacobians=False):
        zeta, q, Js = {}, {}, {}
        inv = [inverse_rule(p) for p in poses]
        for e in self.idx:
            A = self.Xi[e] @ inv[self.tgt[e]]
            z = lin6(A @ poses[self.src[e]])
            zeta[e], q[e] = z, z @ (self.Lam[e] @ z)
            if jacobians:
                Js[e] = np.stack([lin6(A @ GEN[k] @ poses[self.src[e]]) for k in range(6)], axis=1)
        return zeta, q, Js

    def objective(self, q, conf):
        total = 0.0
        for e in self.idx:
            if self.unc[e]:
                l = conf[e]
                total += l * q[e] + self.w * (math.sqrt(l) - 1.0) ** 2
            else:
                total += q[e]
        return total

    def update_confidence(self, q, conf):
        for e in self.idx:
            if self.unc[e]:
                conf[e] = (self.w / (self.w + q[e])) ** 2

    def system(self, n, zeta, Js, conf):
        H, b = np.zeros((n, n)), np.zeros(n)
        for e in self.idx:                                   # edge order: every entry sums its edges in ascending index
            l = conf[e] if self.unc[e] else 1.0
            J, Jt, L = Js[e], -Js[e], self.Lam[e]
            s, t = slice(6 * self.src[e], 6 * self.src[e] + 6), slice(6 * self.tgt[e], 6 * self.tgt[e] + 6)
            H[s, s] += l * (J.T @ L @ J)
            H[s, t] += l * (J.T @ L @ Jt)
            H[t, s] += l * (Jt.T @ L @ J)
            H[t, t] += l * (Jt.T @ L @ Jt)
            b[s] -= l * (J.T @ L @ zeta[e])
            b[t] -= l * (Jt.T @ L @ zeta[e])
        return H, b

    def run(self, poses, conf):
        m, F = self.margins, len(poses)
        n, ref = 6 * F, self.opts["reference_node"]
        ref0 = poses[ref].copy()
        zeta, q, Js = self.residuals(poses, True)
        cur = self.objective(q, conf)
        self.update_confidence(q, conf)
        H, b = self.system(n, zeta, Js, conf)
        lam, nu = 1e-5 * (H.diagonal().max() if n else 0.0), 2.0
        stop = _less(b.max(), 1e-6, m)
        x = np.concatenate([mat2vec(p, m) for p in poses])
        it = solves = 0
        while not stop:
            lm, rho = 0, 0.0
            while True:
                delta = self.solve(H + lam * np.eye(n), b)
                solves += 1
                stop = _less(np.linalg.norm(delta), 1e-6 * (np.linalg.norm(x) + 1e-6), m) or stop
                if not stop:
                    trial = [vec2mat(delta[6 * i:6 * i + 6]) @ poses[i] for i in range(F)]
                    _, q_new, _ = self.residuals(trial)
                    new = self.objective(q_new, conf)
                    rho = (cur - new) / (delta @ (lam * delta + b) + 1e-3)
                    m["rho"].append(abs(rho))
                    if rho > 0:
                        stop = _less(cur - new, 1e-6 * cur, m) or stop
                        if stop:
                            break
                        a = 2.0 * rho - 1.0
                        lam *= max(1.0 / 3.0, min(1.0 - (a * a) * a, 2.0 / 3.0))
                        nu = 2.0
                        cur, poses = new, trial
                        x = np.concatenate([mat2vec(p, m) for p in poses])
                        zeta, q, Js = self.residuals(poses, True)
                        self.update_confidence(q, conf)
                        H, b = self.system(n, zeta, Js, conf)
                        stop = _less(b.max(), 1e-6, m) or stop
                        if stop:
                            break
                    else:
                        m["rejected"] += 1
                        lam *= nu
                        nu *= 2.0
                lm += 1
                stop = stop or lm >= 20
                if rho > 0 or stop:
                    break
            stop = stop or it >= 100 or _less(cur, 1e-6, m)
            it += 1
        comp = ref0 @ inverse_rule(poses[ref])
        return [comp @ p for p in poses], (it, solves, cur, self.w)


def global_optimization_oracle(nodes, edges, solve="numpy", edge_mask=None, **options):
    """-> dict(status, nodes [F,4,4], confidence [E], keep [E] bool, record [12], margins).  `edges`: (source, target, X [E,4,4],
    information [E,6,6], uncertain); fp32 inputs are widened exactly."""
    opts = dict(OPTIONS, **options)
    src, tgt = np.asarray(edges[0], np.int64), np.asarray(edges[1], np.int64)
    X, Lam = np.asarray(edges[2]).astype(np.float64), np.asarray(edges[3]).astype(np.float64)
    unc = np.asarray(edges[4]).astype(bool)
    poses = [p for p in np.asarray(nodes).astype(np.float64)]
    F, E = len(poses), len(src)
    live = np.ones(E, bool) if edge_mask is None else np.asarray(edge_mask).astype(bool).copy()
    margins = {"rho": [], "stop": [], "prune": [], "rejected": 0}
    conf, record = np.ones(E), np.zeros(12)
    record[9:] = live.sum()
    L = np.flatnonzero(live)
    invalid = (not np.isfinite(X[L]).all() or not np.isfinite(Lam[L]).all() or ((src[L] < 0) | (src[L] >= F)).any() or
               ((tgt[L] < 0) | (tgt[L] >= F)).any() or (src[L] == tgt[L]).any() or not np.isfinite(np.array(poses)).all())
    if invalid:
        record[0] = 1
        return dict(status=1, nodes=np.full((F, 4, 4), np.nan), confidence=conf, keep=live, record=record, margins=margins)
    if len(L):
        for p in range(2):
            poses, rec = _Pass((src, tgt, X, Lam, unc), live, opts, SOLVERS[solve], margins).run(poses, conf)
            record[1 + 4 * p:5 + 4 * p] = rec
            for e in np.flatnonzero(live & unc):
                margins["prune"].append(abs(conf[e] - opts["edge_prune_threshold"]))
                live[e] = conf[e] > opts["edge_prune_threshold"]
            record[10 + p] = live.sum()
    return dict(status=0, nodes=np.array(poses), confidence=conf, keep=live, record=record, margins=margins)


def smallest_margin(margins):
    return min([math.inf] + margins["rho"] + margins["stop"] + margins["prune"])


def node_chain_oracle(edges, num_nodes, edge_mask=None):
    """multiway/test_multi_ate.py:129-130 with INVERSE_RULE."""
    odometry, nodes = np.eye(4), [np.eye(4)]
    for e in range(len(edges[0])):
        if edges[4][e] or (edge_mask is not None and not edge_mask[e]) or len(nodes) >= num_nodes:
            continue
        odometry = np.asarray(edges[2][e]).astype(np.float64) @ odometry
        nodes.append(inverse_rule(odometry))
    return np.array(nodes + [np.full((4, 4), np.nan)] * (num_nodes - len(nodes)))


# ---------------------------------------------------------------------------------------------------------------------------
# synthetic graphs
# ---------------------------------------------------------------------------------------------------------------------------
def _motion(rs, deg, metres):
    axis = rs.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    d = rs.standard_normal(3)
    T[:3, 3] = d / np.linalg.norm(d) * metres
    return T


def _information(rs, points):
    """sum of G^T G over `points` random points, G = [-[q]x | I]: what get_information_matrix_from_point_clouds sums."""
    info = np.zeros((6, 6))
    for q in rs.uniform(-1.5, 1.5, (points, 3)):
        G = np.zeros((3, 6))
        G[:, :3] = -np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
        G[:, 3:] = np.eye(3)
        info += G.T @ G
    return info


def synthetic_graph(F, seed, closures=0.5, false_closures=2, odometry_noise=(1.0, 0.01), closure_noise=(0.3, 0.003), fp32=False,
                    node_disturbance=None):
    """A chain of random 25 deg / 0.4 m motions: certain odometry edges (i, i + 1) with `odometry_noise` (deg, m), true loop
    closures with `closure_noise` on about `closures` of the other pairs, `false_closures` gross false ones, information matrices
    from 200-400 random points.  Edges in the driver's order (s ascending, then t).  Nodes: the driver's chain over the odometry
    edges.  fp32: transformations rounded to fp32, as the forward returns them (rotations orthogonal to ~1e-7 only).
    node_disturbance (deg, m): every node but the first is moved that far off the chain -- a start from which Gauss-Newton steps
    overshoot (lin6 saturates at large rotations), so that the LM loop rejects steps (rho <= 0) and raises lambda.
    -> (nodes [F,4,4], edges, false edge indices, true poses)."""
    rs = np.random.RandomState(seed)
    truth = [np.eye(4)]
    for _ in range(F - 1):
        truth.append(truth[-1] @ _motion(rs, 25.0, 0.4))
    others = [(s, t) for s in range(F) for t in range(s + 2, F)]
    chosen = set(i for i in range(len(others)) if rs.random_sample() < closures)
    pool = [i for i in range(len(others)) if i not in chosen]
    false_set = set(rs.choice(pool, min(false_closures, len(pool)), replace=False).tolist()) if pool and false_closures else set()
    src, tgt, X, info, unc, false_idx = [], [], [], [], [], []
    for s in range(F):
        for t in range(s + 1, F):
            exact = np.linalg.inv(truth[t]) @ truth[s]
            if t == s + 1:
                x, u = _motion(rs, *odometry_noise) @ exact, False
            else:
                k = others.index((s, t))
                if k in chosen:
                    x, u = _motion(rs, *closure_noise) @ exact, True
                elif k in false_set:
                    x, u = _motion(rs, rs.uniform(40, 120), rs.uniform(0.5, 1.5)) @ exact, True
                    false_idx.append(len(src))
                else:
                    continue
            src.append(s), tgt.append(t), X.append(x), unc.append(u)
            info.append(_information(rs, int(rs.randint(200, 401))))
    X = np.array(X)
    if fp32:
        X = X.astype(np.float32)
    edges = (np.array(src, np.int32), np.array(tgt, np.int32), X, np.array(info), np.array(unc, bool))
    nodes = node_chain_oracle(edges, F)
    if node_disturbance is not None:
        rs2 = np.random.RandomState(2000 + seed)
        nodes = np.array([nodes[0]] + [_motion(rs2, *node_disturbance) @ p for p in nodes[1:]])
    return nodes, edges, false_idx, np.array(truth)


def exact_graph(F=5, seed=3):
    """Every edge exact, nodes = the truth: nothing to do."""
    nodes, edges, _, truth = synthetic_graph(F, seed, closures=1.0, false_closures=0, odometry_noise=(0.0, 0.0), closure_noise=(0.0, 0.0))
    return truth, edges


# name -> (F, seed, keyword arguments): chosen on the CPU so that every oracle margin is >= MIN_MARGIN
CASES = {
    "f2": (2, 1, dict(closures=0.0, false_closures=0)),
    "f3": (3, 2, dict(closures=1.0, false_closures=0)),
    "f6": (6, 6, dict()),
    "f24": (24, 24, dict()),
    "f57": (57, 57, dict()),
    "reject": (4, 1, dict(node_disturbance=(90.0, 0.3))),        # pass 1 rejects four steps (15 solves, 11 outer iterations)
    "fp32": (7, 7, dict(fp32=True)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    F, seed, kw = CASES[name]
    nodes, edges, false_idx, _ = synthetic_graph(F, seed, **kw)
    return nodes, edges, false_idx


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """Both solve arms of a case, computed once: -> (numpy arm's result, floor)."""
    nodes, edges, _ = case(name)
    a = global_optimization_oracle(nodes, edges, "numpy")
    b = global_optimization_oracle(nodes, edges, "cholesky")
    assert (a["keep"] == b["keep"]).all() and (a["record"][[1, 2, 5, 6]] == b["record"][[1, 2, 5, 6]]).all(), name
    floor = max(np.abs(a["nodes"] - b["nodes"]).max(), np.abs(a["confidence"] - b["confidence"]).max())
    return a, floor


def _check_case_margins(name, oracle):
    m = oracle["margins"]
    assert smallest_margin(m) >= MIN_MARGIN, (name, smallest_margin(m))
    if name == "reject":
        assert m["rejected"] >= 1 and oracle["record"][2] > oracle["record"][1], "pass 1 must reject a step (lambda *= nu)"


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tests: the oracle against cases with known answers, ABI, argument checks
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_exact_graph_stays_put_and_stops_at_once():
    nodes, edges = exact_graph()
    res = global_optimization_oracle(nodes, edges)
    assert res["status"] == 0 and res["keep"].all()
    assert res["record"][1] == 0 and res["record"][2] == 0 and res["record"][5] == 0 and res["record"][6] == 0
    np.testing.assert_allclose(res["nodes"], nodes, rtol=0, atol=1e-12)
    assert res["record"][3] < 1e-20                       # the objective of exact edges
    assert smallest_margin(res["margins"]) >= MIN_MARGIN


@pytest.mark.parametrize("name", ["f6", "f24"])
def test_oracle_prunes_the_false_edges_and_only_them(name):
    nodes, edges, false_idx = case(name)
    res, _ = case_oracle(name)
    assert len(false_idx) == 2
    assert sorted(np.flatnonzero(~res["keep"]).tolist()) == sorted(false_idx)
    assert res["record"][9] == len(edges[0]) and res["record"][11] == len(edges[0]) - 2
    # and the graph is better afterwards: the worst node-pose entry error against the truth shrinks
    F, seed, kw = CASES[name]
    truth = synthetic_graph(F, seed, **kw)[3]
    assert np.abs(res["nodes"] - truth).max() < 0.5 * np.abs(nodes - truth).max()


def test_oracle_is_invariant_under_a_common_motion_of_the_nodes():
    """Residuals see only pose_t^-1 pose_s, so one rigid motion applied to every node (the edges untouched) changes nothing in the
    problem.  The LM iteration itself is not invariant -- lambda damps world-frame increments and |x| enters a stop criterion --
    so the two runs end at two points of the same basin: the relative poses agree to the accuracy of the stop criteria (relative
    objective decrease 1e-6; 1.5e-7 on the poses here), not to rounding.  The prunings are the same."""
    nodes, edges, _ = case("f6")
    W = _motion(np.random.RandomState(8), 70.0, 2.0)
    a, _ = case_oracle("f6")
    b = global_optimization_oracle(np.array([W @ p for p in nodes]), edges)
    assert (a["keep"] == b["keep"]).all()
    for i in range(1, len(nodes)):
        np.testing.assert_allclose(inverse_rule(b["nodes"][0]) @ b["nodes"][i], inverse_rule(a["nodes"][0]) @ a["nodes"][i], rtol=0, atol=1e-5)
    np.testing.assert_allclose(b["nodes"][0], W @ nodes[0], rtol=0, atol=1e-12)       # the reference node is put back
    np.testing.assert_allclose(a["confidence"], b["confidence"], rtol=0, atol=1e-5)


def test_vec2mat_mat2vec_round_trip_and_inverse_rule():
    rs = np.random.RandomState(4)
    for _ in range(20):
        v = np.r_[rs.uniform(-1.5, 1.5, 3), rs.uniform(-2, 2, 3)]
        T = vec2mat(v)
        np.testing.assert_allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-15)
        np.testing.assert_allclose(mat2vec(T), v, rtol=0, atol=1e-14)
        np.testing.assert_allclose(inverse_rule(T) @ T, np.eye(4), atol=1e-14)
    # the generators are the derivatives of vec2mat at zero
    for k in range(6):
        h = np.zeros(6)
        h[k] = 1e-7
        np.testing.assert_allclose((vec2mat(h) - np.eye(4)) / 1e-7, GEN[k], atol=1e-6)
    # INVERSE_RULE is the general inverse, not the transpose: a rotation that is orthogonal to 1e-7 only
    T = vec2mat(np.array([0.3, -0.2, 0.9, 1, 2, 3])).astype(np.float32).astype(np.float64)
    assert np.abs(inverse_rule(T) @ T - np.eye(4)).max() < 1e-15 < np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max()


def test_every_case_has_its_margins():
    for name in CASES:
        if name == "f57":
            continue                                      # 2 s of oracle: the GPU test of that case asserts its margins
        oracle, floor = case_oracle(name)
        _check_case_margins(name, oracle)
        assert oracle["status"] == 0 and floor < 1e-9, (name, floor)


def test_node_chain_oracle():
    nodes, edges, _ = case("f6")
    assert nodes.shape == (6, 4, 4) and (nodes[0] == np.eye(4)).all()
    odo = [i for i in range(len(edges[0])) if not edges[4][i]]
    np.testing.assert_allclose(nodes[2], np.linalg.inv(edges[2][odo[1]] @ edges[2][odo[0]]), atol=1e-14)
    assert np.isnan(node_chain_oracle(edges, 8)[6:]).all()


def test_header_declares_posegraph_entries_and_library_exports_them():
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    assert re.search(r"\bsize_t\s+pdsc_posegraph_workspace_bytes\s*\(", header)
    for name in ("pdsc_posegraph_nodes", "pdsc_global_optimization"):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
    assert "INVERSE_RULE" in header and "SOLVE_RULE" in header
    from pointdsc_amd import _lib, multiway
    assert int(re.search(r"#define\s+PDSC_POSEGRAPH_RECORD\s+(\d+)", header).group(1)) == len(multiway.RECORD_NAMES)
    assert int(re.search(r"#define\s+PDSC_POSEGRAPH_MAX_NODES\s+(\d+)", header).group(1)) == multiway.MAX_NODES
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ("pdsc_posegraph_workspace_bytes", "pdsc_posegraph_nodes", "pdsc_global_optimization"):
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\bT {name}\b", out), name
    # the argument lists of the header and of the binding have the same length
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("pdsc_posegraph_workspace_bytes", "pdsc_posegraph_nodes", "pdsc_global_optimization"):
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", flat, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(",")), name
    lib = _lib.load()
    assert lib.pdsc_version() == int(re.search(r"#define\s+PDSC_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    n = 6 * 57
    assert lib.pdsc_posegraph_workspace_bytes(2, 57, 828) >= 2 * (2 * n * n * 8 + 828 * (36 + 42 + 7) * 8)
    assert lib.pdsc_posegraph_workspace_bytes(0, 57, 828) == 0 and lib.pdsc_posegraph_workspace_bytes(1, multiway.MAX_NODES + 1, 10) == 0
    # argument validation happens before any HIP call
    p = C.c_void_p(16)
    big = 1 << 40
    good = [p] * 7 + [p, p, 0.07, 0.25, 20.0, 0, C.c_void_p(32), p, p, p, None, p, big, 1, 6, 13, 6, 13, None]
    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return lib.pdsc_global_optimization(*a)
    assert call(a0=None) == -1 and b"null pointer" in lib.pdsc_last_error()
    assert call(a6=None, a19=0) == -1 and b"workspace" in lib.pdsc_last_error()       # live_in may be NULL; the workspace may not be short
    assert call(a21=0) == -1 and call(a21=multiway.MAX_NODES + 1) == -1 and b"max_nodes" in lib.pdsc_last_error()
    assert call(a9=float("nan")) == -1 and b"NaN" in lib.pdsc_last_error()
    assert call(a12=6) == -1 and b"reference_node" in lib.pdsc_last_error()
    assert call(a13=p) == -1 and b"alias" in lib.pdsc_last_error()
    assert lib.pdsc_posegraph_nodes(None, p, None, p, p, p, 1, 6, 13, None) == -1
    assert lib.pdsc_posegraph_nodes(p, p, None, p, p, p, 0, 6, 13, None) == -1


def test_posegraph_module_exports_and_argument_checks_on_cpu():
    import pointdsc_amd
    from pointdsc_amd import harness, multiway
    for name in ("pose_graph_nodes", "global_optimization"):
        assert callable(getattr(multiway, name)) and getattr(pointdsc_amd, name) is getattr(multiway, name)
        assert name in pointdsc_amd.__all__ and name in multiway.__all__
    assert callable(harness.multiway_trajectory)
    assert multiway.RECORD_NAMES[0] == "status" and len(multiway.RECORD_NAMES) == 12
    nodes, edges, _ = case("f6")
    tn = torch.from_numpy(nodes)
    te = dict(zip(multiway.EDGE_KEYS, (torch.from_numpy(np.ascontiguousarray(a)) for a in edges)))
    go = multiway.global_optimization
    with pytest.raises(RuntimeError, match="GPU"):
        go(tn, te)
    with pytest.raises(RuntimeError, match="GPU"):
        multiway.pose_graph_nodes(te, 6)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            go(tn, te, max_correspondence_distance=bad)
        with pytest.raises(ValueError, match="finite"):
            go(tn, te, edge_prune_threshold=bad)
    with pytest.raises(ValueError, match="lacks"):
        go(tn, {k: v for k, v in te.items() if k != "information"})
    with pytest.raises(TypeError, match="tuple"):
        go([tn], [(te["source"], te["target"])])
    with pytest.raises(ValueError, match=r"\[E,4,4\]"):
        go(tn, dict(te, transformation=te["transformation"][:, :3]))
    with pytest.raises(ValueError, match=r"\[E\]"):
        go(tn, dict(te, uncertain=te["uncertain"][:-1]))
    with pytest.raises(TypeError, match="fp32 or fp64"):
        go(tn, dict(te, information=te["information"].to(torch.int32)))
    with pytest.raises(TypeError, match="int32 or int64"):
        go(tn, dict(te, source=te["source"].float()))
    with pytest.raises(ValueError, match=r"\[F,4,4\]"):
        go(tn[:, :3], te)
    with pytest.raises(ValueError, match="same length"):
        go([tn, tn], [te])
    with pytest.raises(ValueError, match="same length"):
        go(tn, [te])
    with pytest.raises(ValueError, match="num_nodes"):
        multiway.pose_graph_nodes(te)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def _dev_graph(name, fp32=None):
    nodes, edges, _ = case(name)
    dev = torch.device("cuda:0")
    X = torch.from_numpy(np.ascontiguousarray(edges[2])).to(dev)          # fp32 for the "fp32" case: widened by the wrapper
    assert X.dtype == (torch.float32 if name == "fp32" else torch.float64)
    return torch.from_numpy(nodes).to(dev), {"source": torch.from_numpy(edges[0]).to(dev), "target": torch.from_numpy(edges[1]).to(dev),
                                             "transformation": X, "information": torch.from_numpy(edges[3]).to(dev),
                                             "uncertain": torch.from_numpy(edges[4]).to(dev)}


@functools.lru_cache(maxsize=None)
def device_alone(name):
    """A case run on its own on the device, once: numpy copies of (nodes, confidence, keep, record)."""
    from pointdsc_amd import global_optimization
    nodes, edges = _dev_graph(name)
    res = global_optimization(nodes, edges, **OPTIONS)
    return tuple(res[k].cpu().numpy() for k in ("nodes", "confidence", "keep", "record"))


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_global_optimization_against_the_oracle(name):
    """Per graph: status, final live mask, outer iterations and solves of both passes equal the oracle's; confidences and node
    poses within 100 x the floor of the oracle's two solve arms."""
    oracle, floor = case_oracle(name)
    _check_case_margins(name, oracle)
    nodes, conf, keep, rec = device_alone(name)
    err = max(np.abs(nodes - oracle["nodes"]).max(), np.abs(conf - oracle["confidence"]).max())
    print(f"{name}: F {len(nodes)} E {len(conf)} floor {floor:.3g} observed {err:.3g} (allowed {100 * floor:.3g}); margin "
          f"{smallest_margin(oracle['margins']):.3g}; oracle record {oracle['record'].tolist()}; device record {rec.tolist()}")
    assert rec[0] == 0 == oracle["status"]
    assert (keep == oracle["keep"]).all()
    assert rec[[1, 2, 5, 6]].tolist() == oracle["record"][[1, 2, 5, 6]].tolist()
    assert rec[9:].tolist() == oracle["record"][9:].tolist()
    np.testing.assert_allclose(rec[[3, 4, 7, 8]], oracle["record"][[3, 4, 7, 8]], rtol=1e-9, atol=1e-20)
    assert err <= 100 * floor, (name, err, floor)


@pytest.mark.gpu
def test_ragged_batch_is_bit_identical_to_each_graph_alone():
    from pointdsc_amd import global_optimization
    names = list(CASES)
    graphs = [_dev_graph(n) for n in names]
    res = global_optimization([g[0] for g in graphs], [g[1] for g in graphs], **OPTIONS)
    assert res["record"].shape == (len(names), 12)
    for i, n in enumerate(names):
        nodes, conf, keep, rec = device_alone(n)
        assert _same_bits(res["nodes"][i].cpu().numpy(), nodes), n
        assert _same_bits(res["confidence"][i].cpu().numpy(), conf), n
        assert _same_bits(res["keep"][i].cpu().numpy(), keep), n
        assert _same_bits(res["record"][i].cpu().numpy(), rec), n


@pytest.mark.gpu
def test_graph_replay_is_bit_identical():
    from pointdsc_amd import multiway
    names = ["f6", "f3", "reject"]
    graphs = [_dev_graph(n) for n in names]
    o = OPTIONS
    call = multiway._posegraph_call([g[0] for g in graphs], [g[1] for g in graphs], None, o["max_correspondence_distance"],
                                    o["edge_prune_threshold"], o["preference_loop_closure"], o["reference_node"])
    multiway._posegraph_launch(call)                       # eager: also the one-time LDS opt-in of the kernel
    torch.cuda.synchronize()
    eager = [call[k].clone() for k in ("nodes_out", "confidence", "keep", "record")]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        multiway._posegraph_launch(call)
    for _ in range(2):
        for k in ("nodes_out", "confidence", "keep", "record"):
            call[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, want in zip(("nodes_out", "confidence", "keep", "record"), eager):
            assert _same_bits(call[k].cpu().numpy(), want.cpu().numpy()), k
    nodes, _, _, rec = device_alone("f6")
    assert _same_bits(call["nodes_out"][:6].cpu().numpy().reshape(6, 4, 4), nodes) and _same_bits(call["record"][0].cpu().numpy(), rec)


@pytest.mark.gpu
def test_masked_edges_are_bit_identical_to_the_graph_without_them():
    from pointdsc_amd import global_optimization
    nodes, edges = _dev_graph("f24")
    E = int(edges["source"].shape[0])
    unc = np.flatnonzero(case("f24")[1][4])
    drop = unc[[1, 5, len(unc) // 2, len(unc) - 1]]
    mask = torch.ones(E, dtype=torch.bool, device=nodes.device)
    mask[torch.from_numpy(drop).to(nodes.device)] = False
    masked = global_optimization(nodes, edges, edge_mask=mask, **OPTIONS)
    kept = torch.from_numpy(np.setdiff1d(np.arange(E), drop)).to(nodes.device)
    fewer = global_optimization(nodes, {k: v[kept] for k, v in edges.items()}, **OPTIONS)
    assert _same_bits(masked["nodes"].cpu().numpy(), fewer["nodes"].cpu().numpy())
    assert _same_bits(masked["confidence"][kept].cpu().numpy(), fewer["confidence"].cpu().numpy())
    assert _same_bits(masked["keep"][kept].cpu().numpy(), fewer["keep"].cpu().numpy())
    assert _same_bits(masked["record"].cpu().numpy(), fewer["record"].cpu().numpy())
    assert not masked["keep"].cpu().numpy()[drop].any() and (masked["confidence"].cpu().numpy()[drop] == 1.0).all()
    assert masked["record"][9].item() == E - len(drop)
    # and it is not the unmasked graph's result
    assert not _same_bits(masked["nodes"].cpu().numpy(), device_alone("f24")[0])


@pytest.mark.gpu
def test_invalid_graph_is_nan_and_leaves_its_neighbours_alone():
    from pointdsc_amd import global_optimization
    a, b, c = _dev_graph("f6"), _dev_graph("f6"), _dev_graph("f3")
    bad = dict(b[1], transformation=b[1]["transformation"].clone())
    bad["transformation"][4, 1, 2] = float("nan")
    res = global_optimization([a[0], b[0], c[0]], [a[1], bad, c[1]], **OPTIONS)
    rec = res["record"].cpu().numpy()
    assert rec[:, 0].tolist() == [0, 1, 0]
    assert torch.isnan(res["nodes"][1]).all() and res["keep"][1].all() and (res["confidence"][1] == 1).all()
    for i, n in ((0, "f6"), (2, "f3")):
        nodes, conf, keep, r = device_alone(n)
        assert _same_bits(res["nodes"][i].cpu().numpy(), nodes) and _same_bits(res["confidence"][i].cpu().numpy(), conf)
        assert _same_bits(res["keep"][i].cpu().numpy(), keep) and _same_bits(rec[i], r)
    # the NaN edge masked out: the graph is valid again
    mask = torch.ones(13, dtype=torch.bool, device=a[0].device)
    mask[4] = False
    ok = global_optimization(b[0], bad, edge_mask=mask, **OPTIONS)
    assert ok["record"][0].item() == 0 and torch.isfinite(ok["nodes"]).all()
    # other invalid graphs: an index outside [0, F), s == t, a non-finite node
    for key, value in (("source", 6), ("target", -1), ("target", int(b[1]["source"][4]))):
        e = dict(b[1], **{key: b[1][key].clone()})
        e[key][4] = value
        r = global_optimization(b[0], e, **OPTIONS)
        assert r["record"][0].item() == 1 and torch.isnan(r["nodes"]).all(), (key, value)
    nan_nodes = b[0].clone()
    nan_nodes[3, 0, 3] = float("inf")
    assert global_optimization(nan_nodes, b[1], **OPTIONS)["record"][0].item() == 1


@pytest.mark.gpu
def test_graph_without_live_edges_returns_its_nodes():
    from pointdsc_amd import global_optimization
    nodes, edges = _dev_graph("f6")
    res = global_optimization(nodes, edges, edge_mask=torch.zeros(13, dtype=torch.bool, device=nodes.device), **OPTIONS)
    assert _same_bits(res["nodes"].cpu().numpy(), nodes.cpu().numpy())
    assert res["record"].cpu().numpy().tolist() == [0.0] * 12 and not res["keep"].any()
    none = {k: v[:0] for k, v in edges.items()}
    res = global_optimization(nodes, none, **OPTIONS)
    assert _same_bits(res["nodes"].cpu().numpy(), nodes.cpu().numpy()) and res["confidence"].numel() == 0


@pytest.mark.gpu
def test_pose_graph_nodes_against_the_oracle_chain():
    from pointdsc_amd import pose_graph_nodes
    for name in ("f6", "fp32", "f24"):
        nodes, edges = _dev_graph(name)
        want = case(name)[0]
        got = pose_graph_nodes(edges, len(want)).cpu().numpy()
        assert got.shape == want.shape and (got[0] == np.eye(4)).all()
        np.testing.assert_allclose(got, want, rtol=0, atol=4 * 2.0 ** -52 * max(1.0, np.abs(want).max()) * len(want))
    # a list of graphs, a mask, and more nodes than the chain reaches
    (_, e6), (_, e3) = _dev_graph("f6"), _dev_graph("f3")
    mask = torch.ones(13, dtype=torch.bool, device=e6["source"].device)
    first_odometry = int(np.flatnonzero(~case("f6")[1][4])[0])
    mask[first_odometry] = False
    got = pose_graph_nodes([e6, e3], [6, 4], edge_mask=[mask, torch.ones(3, dtype=torch.bool, device=mask.device)])
    want = node_chain_oracle(case("f6")[1], 6, mask.cpu().numpy())
    assert np.isnan(want[5]).all() and torch.isnan(got[0][5]).all()
    np.testing.assert_allclose(got[0][:5].cpu().numpy(), want[:5], rtol=0, atol=1e-14)
    assert torch.isnan(got[1][3]).all() and torch.isfinite(got[1][:3]).all()


@pytest.mark.gpu
def test_multiway_trajectory_end_to_end_against_the_oracle():
    """harness.multiway_trajectory on 4 demo views with stand-in descriptors: the ATE equals the ATE of the oracle fed with the
    same device edges, within 1e-6 cm."""
    from pointdsc_amd import PointDSC, harness, workloads
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    model = PointDSC(**dict(workloads.BASE_MODEL))
    model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    model = model.eval().cuda()
    views = harness.demo_views(cloud, 4)
    res = harness.multiway_trajectory(model, views, return_graph=True)
    g = res["graph"]
    edges = tuple(g["edges"][k].cpu().numpy() for k in ("source", "target", "transformation", "information", "uncertain"))
    mask = g["edge_mask"].cpu().numpy()
    nodes = g["nodes"].cpu().numpy()
    np.testing.assert_allclose(nodes, node_chain_oracle(edges, 4), rtol=0, atol=1e-13)
    oracle = global_optimization_oracle(nodes, edges, edge_mask=mask)
    assert smallest_margin(oracle["margins"]) >= MIN_MARGIN
    assert res["record"].cpu().numpy()[0] == 0 and (res["keep"].cpu().numpy() == oracle["keep"]).all()
    assert res["nodes_before"] == 4 and res["nodes_after"] == 4
    assert res["edges_before"] == int(mask.sum()) and res["edges_after"] == int(oracle["keep"].sum())
    # the driver's ATE of the oracle's nodes: its align() (fp32, as the reference's .float()) of the node origins onto the views' true
    # origins, then sqrt(mean(err^2)) -- the same operations multiway_trajectory applies to the device's nodes
    from pointdsc_amd import align
    truth = np.stack([np.linalg.inv(v["pose"])[:3, 3] for v in views], axis=1)
    _, err = align(np.ascontiguousarray(oracle["nodes"][:, :3, 3].T), truth)
    ate = float(torch.sqrt((err.double() ** 2).mean()))
    assert ate < 20.0                                          # centimetres: the trajectory is a trajectory
    print(f"ATE device {res['ate_cm']:.9f} cm, oracle {ate:.9f} cm; edges {res['edges_before']} -> {res['edges_after']}")
    assert abs(res["ate_cm"] - ate) <= 1e-6
