"""Inputs and device runs of the bit-for-bit record of everything that goes through the 3x3 Kabsch / Jacobi core (csrc/kabsch3.h):
rigid_transform_3d, the solver tail, the seed-solve backward, ICP and the normals.  tools/record_kabsch_bits.py writes the outputs
into tests/golden/kabsch_bits.npz; tests/test_kabsch_bits.py runs the same functions and compares the raw bits.

The inputs come from numpy's RandomState and from +, -, *, / and sqrt on single elements only (no sum, no matmul, no sin / cos), so
every machine regenerates the same bits and the golden file holds outputs alone."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GOLDEN = Path(__file__).resolve().parent / "golden" / "kabsch_bits.npz"
RIGID_BS, RIGID_N, RIGID_THRESHOLD = 12, 8, 0.5
TAIL_BS, TAIL_N, TAIL_S, TAIL_ITERS, TAIL_KS = 2, 64, 4, 10, (8, 20)
TAIL_SIGMA, TAIL_SIGMA_SPAT, REFINE_THRESHOLD = 1.5, 0.1, 0.1
RANK0_SEED = (1, 2)                                  # (pair, seed) whose neighbour list is k copies of one index: H is rounding residue
RANK1_SEED = (0, 1)                                  # (pair, seed) whose neighbours have src y = z = 0: rows 1, 2 of H are exactly 0
RIGID_RANK1, RIGID_ZERO = 8, (9, 10)                 # rigid cases whose fp32 H is exactly of rank 1 / exactly 0
ICP_FIXTURE = "n1000_s1"                             # the smallest case of tests/test_icp.py
NORMALS_RADIUS, NORMALS_MAX_NN = 0.1, 30


def _rotation(rs):
    """A proper rotation [3,3] fp64 from a random quaternion."""
    w, x, y, z = rs.standard_normal(4)
    n = w * w + x * x + y * y + z * z
    return np.array([[1 - 2 * (y * y + z * z) / n, 2 * (x * y - w * z) / n, 2 * (x * z + w * y) / n],
                     [2 * (x * y + w * z) / n, 1 - 2 * (x * x + z * z) / n, 2 * (y * z - w * x) / n],
                     [2 * (x * z - w * y) / n, 2 * (y * z + w * x) / n, 1 - 2 * (x * x + y * y) / n]])


def _moved(A, R, t):
    """R a + t for the rows a of A (fp64, written out: no matmul)."""
    return np.stack([(R[i, 0] * A[:, 0] + R[i, 1] * A[:, 1]) + R[i, 2] * A[:, 2] + t[i] for i in range(3)], axis=1)


def rigid_inputs():
    """A, B [12,8,3], weights [12,8] fp32: 0-3 rigid pairs, 4-5 with noise, 6 coplanar (rank 2), 7 a reflection (the det correction),
    8 collinear (integers s d about the origin: H = 60 d d'^T exactly, the rank <= 1 fallback with a real u1), 9 all points equal
    (A at the origin, so H == 0 exactly), 10 all weights zero, 11 random weights in (0, 1) (what weight_threshold = 0.5 cuts)."""
    rs = np.random.RandomState(20261)
    A = rs.standard_normal((RIGID_BS, RIGID_N, 3))
    B = np.empty_like(A)
    W = np.ones((RIGID_BS, RIGID_N))
    A[6, :, 2] = 0.0
    A[RIGID_RANK1] = np.array([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0])[:, None] * np.array([2.0, -1.0, 3.0])
    A[9] = 0.0
    for b in range(RIGID_BS):
        R, t = _rotation(rs), rs.standard_normal(3)
        if b == 7:
            R = R * np.array([[1.0], [1.0], [-1.0]])
        if b == RIGID_RANK1:      # small integers about the origin, a signed permutation, t = 0: centroids and H are exact in fp32
            R, t = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]), np.zeros(3)
        B[b] = _moved(A[b], R, t)
    for b in (4, 5, 11):
        B[b] += 0.01 * rs.standard_normal((RIGID_N, 3))
    W[10] = 0.0
    W[11] = rs.uniform(0.05, 0.95, RIGID_N)
    return tuple(torch.from_numpy(np.ascontiguousarray(x, np.float32)) for x in (A, B, W))


def tail_inputs(k):
    """bs 2, N 64, S 4: unit feature rows around one common direction per pair, 70 % of the correspondences a rigid motion with
    1 cm noise, neighbour lists of k distinct rows -- but RANK0_SEED's, which is k copies of one row (rank 0 in exact arithmetic; in fp32 H is a residue of full rank); RANK1_SEED's rows have src y = z = 0,
    so whatever the weights its centred src has y = z = 0 and rows 1, 2 of its H are exactly zero (the rank <= 1 fallback with
    u1 = (+-1, 0, 0)) -- and an upstream gradient that is non-zero for every seed."""
    rs = np.random.RandomState(20262 + k)
    f = 0.35 * rs.standard_normal((TAIL_BS, TAIL_N, 128)) + rs.standard_normal((TAIL_BS, 1, 128))
    normed = f / np.sqrt(np.cumsum(f * f, axis=-1)[..., -1:])
    src = rs.uniform(-0.5, 0.5, (TAIL_BS, TAIL_N, 3))
    rank1_rows = rs.permutation(TAIL_N)[:k]
    src[RANK1_SEED[0], rank1_rows, 1:] = 0.0
    tgt = np.empty_like(src)
    for b in range(TAIL_BS):
        tgt[b] = _moved(src[b], _rotation(rs), 0.3 * rs.standard_normal(3)) + 0.01 * rs.standard_normal((TAIL_N, 3))
        out = rs.permutation(TAIL_N)[: (3 * TAIL_N) // 10]
        tgt[b, out] = rs.uniform(-0.5, 0.5, (len(out), 3))
    knn = np.stack([np.stack([rs.permutation(TAIL_N)[:k] for _ in range(TAIL_S)]) for _ in range(TAIL_BS)])
    knn[RANK0_SEED] = 17
    knn[RANK1_SEED] = rank1_rows
    dtrans = rs.standard_normal((TAIL_BS, TAIL_S, 4, 4))
    dtrans[:, :, 3] = 0.0
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32))      # noqa: E731
    return {"normed": t32(normed), "src": t32(src), "tgt": t32(tgt), "knn": torch.from_numpy(np.ascontiguousarray(knn, np.int32)),
            "dtrans": t32(dtrans), "sigma": torch.tensor([TAIL_SIGMA]), "sigma_spat": torch.tensor([TAIL_SIGMA_SPAT])}


def normals_cloud():
    """[1,64,3] fp32: 31 scattered points, a planar patch of 30 (z = 0.3) and three collinear points far from the rest."""
    rs = np.random.RandomState(20263)
    scattered = rs.uniform(0.0, 0.2, (31, 3))
    patch = np.concatenate([rs.uniform(0.5, 0.62, (30, 2)), np.full((30, 1), 0.3)], axis=1)
    line = np.array([2.0, 2.0, 2.0]) + np.arange(3.0)[:, None] * np.array([0.01, 0.02, 0.03])
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([scattered, patch, line]), np.float32))[None]


# ---- the body of csrc/kabsch3.h in Python floats (IEEE fp64, the source's operation order) -------------------------------------
def kabsch_port(H, cA=(0.0, 0.0, 0.0), cB=(0.0, 0.0, 0.0)):
    """H [3][3], cA, cB as the kernel holds them (fp32 values) -> (T [4][4] fp64 before the output rounding, branch): branch is
    "full" (n2 > 1e-12 n1), "rank1" (the rank <= 1 fallback with a real u1: n1 > 1e-150) or "zero" (n1 <= 1e-150: u1 = e_x).
    Says which branch an input takes, and gives the bits of an exact input (what the record of such a case is checked against)."""
    from math import sqrt
    H = [[float(x) for x in row] for row in H]
    A = [[H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j] for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(12):
        off = abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2])
        diag = abs(A[0][0]) + abs(A[1][1]) + abs(A[2][2])
        if off <= 1e-300 or off <= 1e-17 * diag:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if abs(apq) < 1e-300:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            tt = (1.0 if theta >= 0 else -1.0) / (abs(theta) + sqrt(theta * theta + 1.0))
            c = 1.0 / sqrt(tt * tt + 1.0)
            s = tt * c
            for r in range(3):
                arp, arq = A[r][p], A[r][q]
                A[r][p], A[r][q] = c * arp - s * arq, s * arp + c * arq
            for r in range(3):
                apr, aqr = A[p][r], A[q][r]
                A[p][r], A[q][r] = c * apr - s * aqr, s * apr + c * aqr
            for r in range(3):
                vrp, vrq = V[r][p], V[r][q]
                V[r][p], V[r][q] = c * vrp - s * vrq, s * vrp + c * vrq
    i0, i1, i2 = 0, 1, 2
    e0, e1, e2 = A[0][0], A[1][1], A[2][2]
    if e0 < e1:
        e0, e1, i0, i1 = e1, e0, i1, i0
    if e0 < e2:
        e0, e2, i0, i2 = e2, e0, i2, i0
    if e1 < e2:
        e1, e2, i1, i2 = e2, e1, i2, i1
    v1, v2 = [V[r][i0] for r in range(3)], [V[r][i1] for r in range(3)]
    v3 = [v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]]
    u1 = [H[i][0] * v1[0] + H[i][1] * v1[1] + H[i][2] * v1[2] for i in range(3)]
    n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2])
    u1 = [x / n1 for x in u1] if n1 > 1e-150 else [1.0, 0.0, 0.0]
    u2 = [H[i][0] * v2[0] + H[i][1] * v2[1] + H[i][2] * v2[2] for i in range(3)]
    dp = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2]
    u2 = [u2[i] - dp * u1[i] for i in range(3)]
    n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2])
    if n2 > 1e-12 * (n1 if n1 > 1e-150 else 1.0) and n2 > 1e-150:
        branch = "full"
        u2 = [x / n2 for x in u2]
    else:
        branch = "rank1" if n1 > 1e-150 else "zero"
        a = [abs(x) for x in u1]
        m = 0 if (a[0] <= a[1] and a[0] <= a[2]) else (1 if a[1] <= a[2] else 2)
        e = [1.0 if m == i else 0.0 for i in range(3)]
        d2 = e[0] * u1[0] + e[1] * u1[1] + e[2] * u1[2]
        u2 = [e[i] - d2 * u1[i] for i in range(3)]
        n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2])
        u2 = [x / n2 for x in u2]
    u3 = [u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]]
    R = [[v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j] for j in range(3)] for i in range(3)]
    T = [R[i] + [float(cB[i]) - (R[i][0] * float(cA[0]) + R[i][1] * float(cA[1]) + R[i][2] * float(cA[2]))] for i in range(3)]
    return T + [[0.0, 0.0, 0.0, 1.0]], branch


def rigid_covariance(A, B, W, threshold=0.0):
    """rigid_transform_kernel's fp32 sums for one problem of n <= 64 points (one point per lane; exact for RIGID_RANK1 and
    RIGID_ZERO, whose every partial sum is exact, and within rounding for the others) -> (H [3][3], cA [3], cB [3]) fp32."""
    f = np.float32
    A, B, w = A.numpy().astype(f), B.numpy().astype(f), W.numpy().astype(f).copy()
    w[w < f(threshold)] = 0
    den = f(np.cumsum(w)[-1] + f(1e-6))
    cA = [f(np.cumsum(A[:, r] * w)[-1] / den) for r in range(3)]
    cB = [f(np.cumsum(B[:, r] * w)[-1] / den) for r in range(3)]
    am, bm = A - np.array(cA, f), B - np.array(cB, f)
    H = [[f(np.cumsum(am[:, r] * w * bm[:, c])[-1]) for c in range(3)] for r in range(3)]
    return H, cA, cB


# ---- device runs: name -> CPU tensor -------------------------------------------------------------------------------------------
def _g(t):
    return t.to("cuda:0")


def run_rigid():
    from pointdsc_amd import ops
    A, B, W = (_g(x) for x in rigid_inputs())
    return {"rigid.T": ops.rigid_transform_3d(A, B, W).cpu(),
            "rigid.T_threshold": ops.rigid_transform_3d(A, B, W, weight_threshold=RIGID_THRESHOLD).cpu()}


@functools.lru_cache(maxsize=None)
def run_tail(k):
    """The solver tail and its backward on one data set (computed once, shared by the tests, left unchanged)."""
    from pointdsc_amd import ops
    inp = tail_inputs(k)
    nd, src, tgt, knn = _g(inp["normed"]), _g(inp["src"]), _g(inp["tgt"]), _g(inp["knn"])
    sg, sd = _g(inp["sigma"]), _g(inp["sigma_spat"])
    iters, mask, _ = ops.seed_power_iteration(nd, src, tgt, knn, sg, sd, TAIL_ITERS)
    trans, w = ops.seed_transforms(src, tgt, knn, iters, mask, TAIL_ITERS)                     # kabsch_batch_kernel
    _, mask2, trans2, w2, _ = ops.seed_solve(nd, src, tgt, knn, sg, sd, TAIL_ITERS)            # fixup_kabsch_kernel
    final, solves = ops.post_refinement(trans2[:, 0].contiguous(), src, tgt, REFINE_THRESHOLD)  # refine_kernel
    dnormed, dsigma = ops.seed_solve_backward(nd, src, tgt, knn, sg, sd, mask, TAIL_ITERS, _g(inp["dtrans"]))
    # RANK1_SEED's s' = (s1, 0, 0) makes its own gradient, and so dsigma, NaN: a second run without its upstream gradient keeps
    # the other seeds' dsigma pinned
    rest = inp["dtrans"].clone()
    rest[RANK1_SEED] = 0.0
    dnormed_rest, dsigma_rest = ops.seed_solve_backward(nd, src, tgt, knn, sg, sd, mask, TAIL_ITERS, _g(rest))
    out = {"transforms.trans": trans, "transforms.w": w, "transforms.mask": mask, "solve.trans": trans2, "solve.w": w2,
           "solve.mask": mask2, "refine.final": final, "refine.solves": solves, "backward.dnormed": dnormed, "backward.dsigma": dsigma,
           "backward_rest.dnormed": dnormed_rest, "backward_rest.dsigma": dsigma_rest}
    return {f"tail_k{k}.{name}": t.cpu() for name, t in out.items()}


def run_icp():
    import test_icp as TI
    d = np.load(TI.GOLDEN / f"{ICP_FIXTURE}.npz")
    got = TI._gpu_run([d["src_keypts"][0]], [d["tgt_keypts"][0]], [d["ref_final_trans"][0]])
    return {f"icp.{name}": torch.from_numpy(np.ascontiguousarray(got[name]))
            for name in ("transformation_f64", "transformation", "fitness", "inlier_rmse", "num_correspondences", "iterations")}


def run_normals():
    from pointdsc_amd import features
    return {"normals": features.estimate_normals(_g(normals_cloud()), NORMALS_RADIUS, NORMALS_MAX_NN).cpu()}


def bits(t):
    """The raw bits of a CPU tensor as an integer tensor of the same shape (NaN payloads included)."""
    t = t.contiguous()
    return t if not t.is_floating_point() else t.view({4: torch.int32, 8: torch.int64}[t.element_size()])
