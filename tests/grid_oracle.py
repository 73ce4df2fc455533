"""f-20: test infrastructure of tests/test_grid_search.py -- the exact brute-force oracles of the radius search of
csrc/icp_grid.h (nearest target within a radius; neighbour lists) and of the voxel keys of csrc/voxel.hip, the case builders, and
a switchable numpy model of the cell grid, of the streaming selection of nb_search_kernel and of the voxel index.

Most cases are DYADIC: every coordinate is a multiple of 2^-10 with |coordinate| <= 2^9 and the squared radius is exact in fp32
(or no distance comes near it), so every difference, square and three-term sum of a squared distance is exact in fp64: ties are
exact ties, the oracle is plain brute force without any margin condition, and index lists, counts and d2 are compared with
assert_array_equal.  Sums (information matrix, sum d2, voxel means) are formed from integers and rounded once.

The model restates what the header does -- box, cell width, cap, cells per axis, hash, clamp, 27-cell walk -- with the constants
read from the sources by regex, and takes a set of seeded DEFECTS.  It serves two CPU checks: every case reaches the branch it is
listed for, and every defect is rejected by at least one case (a defect no case rejects means a case is missing).
"""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointdsc_amd" / "csrc"

Q10 = 2.0 ** -10                                    # the quantum of the dyadic cases
POSE_SHIFT = (0.125, -0.25, 0.5)                    # the pure dyadic translation of the second run of every A case


# ---------------------------------------------------------------------------------------------------------------------------
# constants of the sources, by regex: a changed constant fails the branch-reach test instead of silently moving a case
# ---------------------------------------------------------------------------------------------------------------------------
def _const(text, name, cast=float):
    m = re.search(rf"constexpr\s+\w+(?:\s+\w+)?\s+{name}\s*=\s*([-+0-9.eE]+)", text)
    assert m, name
    return cast(m.group(1))


def source_constants():
    grid = (CSRC / "icp_grid.h").read_text()
    voxel = (CSRC / "voxel.hip").read_text()
    fpfh = (CSRC / "fpfh.hip").read_text()
    many = (CSRC / "cloud_many.h").read_text()
    primes = re.search(r"cx \* (\d+)u \^ \(unsigned\)cy \* (\d+)u \^ \(unsigned\)cz \* (\d+)u", grid)
    hmin = re.search(r"int h = (\d+);\s*while \(h < 2 \* nt\) h <<= 1;", grid)
    assert primes and hmin
    return {"cell_margin": _const(grid, "ICP_CELL_MARGIN"), "max_cells": _const(grid, "ICP_MAX_CELLS_PER_AXIS"),
            "tile": _const(grid, "ICP_NT", int), "primes": tuple(int(p) for p in primes.groups()), "hash_min": int(hmin.group(1)),
            "voxel_max": _const(voxel, "VOXEL_MAX_PER_AXIS"), "cap": _const(fpfh, "FPFH_CAP", int),
            "wave": _const(fpfh, "FPFH_WAVE", int), "chunk": _const(many, "CLOUD_CHUNK", int)}


# ---------------------------------------------------------------------------------------------------------------------------
# exact brute-force oracles (numpy fp64)
# ---------------------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).astype(np.float64)


def radius2(r):
    """FLANN_RADIUS_RULE: the squared radius rounded to fp32, compared with a strict '<' against the fp64 distance."""
    return float(np.float32(r * r))


def sqdist(P, Q):
    """[len(P), len(Q)] fp64 squared distances in the kernels' order (dx dx + dy dy) + dz dz."""
    d = P[:, None, :] - Q[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def apply_pose(T, S):
    """Eigen (T (x, y, z, 1)).head<3>() / w in the kernels' order; an identity pose is not applied (Eigen isIdentity())."""
    T = np.asarray(T, np.float32).astype(np.float64)
    if np.array_equal(T, np.eye(4)):
        return S.copy()
    x, y, z = S[:, 0], S[:, 1], S[:, 2]
    w = T[3, 0] * x + T[3, 1] * y + T[3, 2] * z + T[3, 3]
    return np.stack([(T[i, 0] * x + T[i, 1] * y + T[i, 2] * z + T[i, 3]) / w for i in range(3)], axis=1)


def nearest_oracle(P, Q, r):
    """Nearest target with d2 < float32(r r) per row of P, the lowest index among equal distances (TIE_RULE); no margin
    condition.  -> corr [len(P)] (-1 = none), d2 of the winner (0 where none)."""
    d2 = sqdist(P, Q)
    ok = d2 < radius2(r)
    masked = np.where(ok, d2, np.inf)
    corr = masked.argmin(axis=1)                       # the first minimum: the lowest index
    best = masked[np.arange(len(P)), corr]
    hit = ok.any(axis=1)
    return np.where(hit, corr, -1), np.where(hit, best, 0.0)


def lists_oracle(P, r, max_nn):
    """search_hybrid of every point of P in P: ascending (d2, index), self included, cut at max_nn.
    -> idx [n,max_nn] (-1 beyond the count), d2 [n,max_nn] (0 beyond), count [n]."""
    d2 = sqdist(P, P)
    ok = d2 < radius2(r)
    masked = np.where(ok, d2, np.inf)
    order = np.argsort(masked, axis=1, kind="stable")[:, :max_nn]       # stable: ascending index among equal d2
    count = np.minimum(ok.sum(axis=1), max_nn)
    n = len(P)
    idx = np.full((n, max_nn), -1, np.int64)
    out = np.zeros((n, max_nn))
    k = order.shape[1]
    valid = np.arange(k)[None, :] < count[:, None]
    idx[:, :k] = np.where(valid, order, -1)
    out[:, :k] = np.where(valid, np.take_along_axis(masked, order, axis=1), 0.0)
    return idx, out, count


def lists_margin(P, r):
    """Smallest relative margin of a discrete decision of the list search of a seeded cloud: the radius test and the order of any
    two candidates of one list (which also covers every cut)."""
    d2 = sqdist(P, P)
    r2 = radius2(r)
    margin = float(np.abs(d2 - r2).min() / r2)
    s = np.sort(np.where(d2 < r2, d2, np.inf), axis=1)
    with np.errstate(invalid="ignore"):                  # inf - inf beyond the end of a list
        gap = np.diff(s, axis=1)
    gap = gap[np.isfinite(gap)]
    return min(margin, float(gap.min() / r2)) if len(gap) else margin


def to_ints(a, quantum):
    """The exact integers a / quantum as a Python-int object array (asserts that a lies on the quantum)."""
    a = np.asarray(a, np.float64)
    k = np.round(a / quantum)
    assert np.array_equal(k * quantum, a), "not on the quantum"
    return np.array([int(v) for v in k.ravel()], dtype=object).reshape(a.shape)


def info_rows_int(Qi, one):
    """The three rows g of every target, as integers in units of the quantum (the entry 1 is `one` = 1 / quantum)."""
    out = []
    for x, y, z in Qi:
        out.append([[0, z, -y, one, 0, 0], [-z, 0, x, 0, one, 0], [y, -x, 0, 0, 0, one]])
    return out


def info_exact(Q, corr, quantum):
    """The information matrix of the matched targets from integers, rounded once.  -> info [6,6] fp64, bits: the largest over the
    entries of the bit length of sum |terms| counted from the lowest set bit of any term of the entry (every partial sum of every
    order is a multiple of that bit and below sum |terms|, so <= 53 means that every order of summation is exact)."""
    Qi = to_ints(Q[corr[corr >= 0]], quantum)
    one = int(round(1.0 / quantum))
    tot = [[0] * 6 for _ in range(6)]
    mag = [[0] * 6 for _ in range(6)]
    low = [[0] * 6 for _ in range(6)]
    for rows in info_rows_int(Qi, one):
        for g in rows:
            for a in range(6):
                if g[a] == 0:
                    continue
                for b in range(6):
                    t = g[a] * g[b]
                    tot[a][b] += t
                    mag[a][b] += abs(t)
                    low[a][b] |= abs(t)
    info = np.array([[float(v) * quantum * quantum for v in row] for row in tot])
    bits = max(_span(mag[a][b], low[a][b]) for a in range(6) for b in range(6))
    return info, bits


def _span(magnitude, any_bits):
    """Bits between the top bit of `magnitude` and the lowest set bit of `any_bits` (the OR of the terms)."""
    if not any_bits:
        return 0
    return (magnitude >> ((any_bits & -any_bits).bit_length() - 1)).bit_length()


def sum_d2_exact(P, Q, corr, quantum):
    """sum of the winners' squared distances from integers -> (the sum rounded once, its bit span as in info_exact)."""
    sel = corr >= 0
    if not sel.any():
        return 0.0, 0
    d = to_ints(P[sel], quantum) - to_ints(Q[corr[sel]], quantum)
    terms = [int(v[0]) ** 2 + int(v[1]) ** 2 + int(v[2]) ** 2 for v in d]
    total, low = sum(terms), 0
    for t in terms:
        low |= t
    return float(total) * quantum * quantum, _span(total, low)


# ---------------------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------------------
def lattice(n, step, origin):
    """n^3 lattice, index (ix n + iy) n + iz."""
    g = np.arange(n) * step
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return (np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1) + np.asarray(origin)).astype(np.float32)


LATTICE_ORIGIN = (-1.25, -0.75, -2.0)
# the seeds of the fp32 cases, each the first of 0, 1, 2, .. whose oracle margins (both poses; A4 and A5 also as clouds searched
# against themselves) are >= NEAR_TIE: test_seeded_cases_keep_their_margins asserts it
SEED_CAP, SEED_SPARSE, SEED_OFFSET = 0, 0, 0


def case_on_lattice():
    o = np.asarray(LATTICE_ORIGIN)
    return {"name": "A1 on-lattice", "Q": lattice(6, 0.25, o), "S": lattice(12, 0.25, o - 0.75), "r": 0.5, "quantum": Q10}


def case_shifted_lattice():
    o = np.asarray(LATTICE_ORIGIN)
    return {"name": "A2 shifted lattice", "Q": lattice(6, 0.25, o), "S": lattice(12, 0.25, o - 0.75 + 0.125), "r": 0.51,
            "quantum": Q10}


def case_radius_shell():
    """27 isolated targets on a coarse lattice of spacing 2.5 with seeded dyadic phases in [0, 0.5) (so >= 2.0 = 4 r apart, and
    at varied positions inside their cells); per target 6 sources at exactly r (excluded) and 6 at r - 2^-10 (included)."""
    rs = np.random.RandomState(20)
    r = 0.5
    base = lattice(3, 2.5, (-3.0, 1.0, -6.5)).astype(np.float64)
    Q = base + rs.randint(0, 32, base.shape) / 64.0
    S = []
    for q in Q:
        for axis in range(3):
            for sign in (1.0, -1.0):
                for d in (r, r - Q10):
                    p = q.copy()
                    p[axis] += sign * d
                    S.append(p)
    return {"name": "A3 radius shell", "Q": Q.astype(np.float32), "S": np.array(S, np.float32), "r": r, "quantum": Q10}


def case_cell_cap(seed=SEED_CAP):
    """Two clusters of 40 targets (cubes of edge 0.05) at x = -2000 and x = +2000; two noisy copies of every target as sources."""
    rs = np.random.RandomState(1000 + seed)
    r = 1e-3
    Q = rs.uniform(0.0, 0.05, (80, 3))
    Q[:40, 0] -= 2000.0
    Q[40:, 0] += 2000.0
    Q = Q.astype(np.float32)
    S = (np.repeat(Q.astype(np.float64), 2, axis=0) + rs.standard_normal((160, 3)) * 0.3 * r).astype(np.float32)
    return {"name": "A4 cell cap", "Q": Q, "S": S, "r": r, "quantum": None}


def case_sparse_wide(seed=SEED_SPARSE):
    rs = np.random.RandomState(2000 + seed)
    Q = rs.uniform(-80.0, 80.0, (20, 3)).astype(np.float32)
    S = (np.repeat(Q.astype(np.float64), 8, axis=0) + rs.standard_normal((160, 3)) * 0.05).astype(np.float32)
    return {"name": "A5 sparse and wide", "Q": Q, "S": S, "r": 0.1, "quantum": None}


def _probe_sources(centre, r):
    """Dyadic probes around a point: on it, inside r, exactly at r (excluded), just inside, outside, diagonal."""
    off = [(0, 0, 0), (0.25, 0, 0), (0, -0.25, 0.25), (r, 0, 0), (0, -r, 0), (0, 0, r), (r - Q10, 0, 0), (0, 0, -(r - Q10)),
           (0.75, 0, 0), (0, 1.5, 0), (-0.25, -0.25, -0.25), (0.375, 0.25, -0.125), (-2.0, 0, 0)]
    return (np.asarray(centre, np.float64) + np.array(off)).astype(np.float32)


def cases_degenerate():
    r = 0.5
    c = np.array([1.5, -2.25, 0.75])
    out = [{"name": "A6a coincident targets", "Q": np.repeat(c[None], 50, 0).astype(np.float32), "S": _probe_sources(c, r)}]
    line = np.stack([-3.0 + 0.25 * np.arange(40), np.full(40, 0.5), np.full(40, -1.25)], 1)
    S = np.concatenate([line + (0.125, 0.25, 0), line + (0, 0, -0.5), line + (0, 0.25, 0.375), line[:4] + (-0.5, 0, 0),
                        line[-4:] + (0.375, -0.25, 0)])
    out.append({"name": "A6b collinear target", "Q": line.astype(np.float32), "S": S.astype(np.float32)})
    gx, gy = np.meshgrid(np.arange(8) * 0.25, np.arange(8) * 0.25, indexing="ij")
    plane = np.stack([gx.ravel() - 1.0, gy.ravel() + 2.0, np.full(64, -0.5)], 1)
    S = np.concatenate([plane + (0.125, 0.125, 0.25), plane + (0, 0, -0.5), plane + (0, 0, 0.5 - Q10), plane + (0.125, 0, -0.375)])
    out.append({"name": "A6c planar target", "Q": plane.astype(np.float32), "S": S.astype(np.float32)})
    out.append({"name": "A6d one target", "Q": c[None].astype(np.float32), "S": _probe_sources(c, r)})
    out.append({"name": "A6e one source", "Q": _probe_sources(c, r), "S": (c + (0.125, 0, 0))[None].astype(np.float32)})
    for k in out:
        k.update(r=r, quantum=Q10)
    return out


def case_fp32_radius():
    """r = 0.05 * 1.4: float32(0.07)^2 lies between r r in fp64 and float32(r r); one fp32 step further out lies beyond both."""
    a = np.float32(0.07)
    b = np.nextafter(a, np.float32(1.0))
    return {"name": "A7 fp32 radius rule", "Q": np.zeros((1, 3), np.float32), "S": np.array([[a, 0, 0], [b, 0, 0]], np.float32),
            "r": 0.05 * 1.4, "quantum": 2.0 ** -27}


def case_large_offset(seed=SEED_OFFSET):
    rs = np.random.RandomState(3000 + seed)
    Q = (np.array([4096.0, -4096.0, 2048.0]) + rs.uniform(0, 1, (200, 3))).astype(np.float32)
    S = (Q.astype(np.float64) + rs.standard_normal((200, 3)) * 0.03).astype(np.float32)
    return {"name": "A8 large offset", "Q": Q, "S": S, "r": 0.07, "quantum": None}


def nearest_cases():
    return ([case_on_lattice(), case_shifted_lattice(), case_radius_shell(), case_cell_cap(), case_sparse_wide()] + cases_degenerate() +
            [case_fp32_radius(), case_large_offset()])


def pose_variants(case):
    """(tag, source fp32, pose fp32): the case as it is under the identity, and with the source moved by -POSE_SHIFT under the
    translation by +POSE_SHIFT."""
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = POSE_SHIFT
    moved = (case["S"].astype(np.float64) - np.asarray(POSE_SHIFT)).astype(np.float32)
    return [("identity", case["S"], np.eye(4, dtype=np.float32)), ("translation", moved, T)]


# ---- B: neighbour lists -------------------------------------------------------------------------------------------------------
def cloud_lattice():
    return lattice(8, 0.25, (-0.75, 1.5, -2.25))


def cloud_coincident():
    c = np.array([0.5, -1.0, 2.0])
    rs = np.random.RandomState(21)
    others = c + rs.randint(-256, 257, (20, 3)) * Q10            # |offset| <= 0.25 per axis: within r = 0.5
    return np.concatenate([np.repeat(c[None], 300, 0), others]).astype(np.float32)


def cloud_crowded(seed=22, origin=(3.0, -1.5, 0.25)):
    rs = np.random.RandomState(seed)
    return (np.asarray(origin) + rs.randint(0, 257, (700, 3)) * Q10).astype(np.float32)


def cloud_many():
    """About 2100 points, three chunks of path many: the lattice, two crowded cubes and 180 far points."""
    rs = np.random.RandomState(23)
    far = rs.randint(-400 * 1024, 400 * 1024, (180, 3)) * Q10
    return np.concatenate([cloud_lattice(), cloud_crowded(), cloud_crowded(24, (11.0, -1.5, 0.25)), far.astype(np.float32)]).astype(np.float32)


def list_cases():
    """name, cloud, r, the max_nn values, quantum (None: seeded fp32)."""
    return [{"name": "B1 lattice", "P": cloud_lattice(), "r": 1.0, "max_nn": (1, 30, 64, 65, 100, 128), "quantum": Q10},
            {"name": "B2 coincident block", "P": cloud_coincident(), "r": 0.5, "max_nn": (128,), "quantum": Q10},
            {"name": "B3 crowded cell", "P": cloud_crowded(), "r": 1.0, "max_nn": (1, 100, 128), "quantum": Q10},
            {"name": "B4 cell cap cloud", "P": case_cell_cap()["Q"], "r": 1e-3, "max_nn": (30,), "quantum": None},
            {"name": "B4 sparse cloud", "P": case_sparse_wide()["Q"], "r": 0.1, "max_nn": (30,), "quantum": None},
            {"name": "B5 many", "P": cloud_many(), "r": 1.0, "max_nn": (100,), "quantum": Q10}]


# ---- C: voxel keys ------------------------------------------------------------------------------------------------------------
def _dyadic_normals(n, seed):
    return np.random.RandomState(seed).randint(-1024, 1025, (n, 3)) * Q10


def voxel_cases():
    """name, points fp32, dyadic normals fp64, voxel, accepted."""
    rs = np.random.RandomState(30)
    faces = (rs.randint(-64, 1, (600, 3)) / 16.0).astype(np.float32)                   # multiples of 1/16 in [-4, 0]
    top = (2 ** 20 - 1) * Q10
    few = np.array([[0, 0, 0], [0.25, 0.5, 0.125], [Q10, 0, 0], [0.25, 0.5, 0.125 + Q10 / 2], [300.0, 0.25, 0], [2 * Q10, 0.5, 0.125]])
    limit = np.concatenate([few, [[top, 0.25, 0.0]]]) + (-512.0, 0, 0)
    beyond = np.concatenate([few, [[top + Q10, 0.25, 0.0]]]) + (-512.0, 0, 0)
    run = np.concatenate([rs.randint(0, 64, (40, 3)) / 8.0 + (0, 0, 1.0),                # a few other voxels before, inside and after
                          np.array([2.0, 3.0, 0.5]) + rs.randint(0, 256, (1500, 3)) * Q10 / 2])
    run = run[rs.permutation(len(run))]
    cases = [{"name": "C1 points on voxel faces", "P": faces, "voxel": 0.125, "accepted": True},
             {"name": "C2 2^20 voxels on x", "P": limit, "voxel": Q10, "accepted": True},
             {"name": "C2 2^20 + 1 voxels on x", "P": beyond, "voxel": Q10, "accepted": False},
             {"name": "C3 long run", "P": run, "voxel": 0.25, "accepted": True}]
    for i, c in enumerate(cases):
        c["P"] = np.asarray(c["P"], np.float32)
        c["normals"] = _dyadic_normals(len(c["P"]), 40 + i)
    return cases


def voxel_model(P, voxel, voxel_max, defects=()):
    """The keys of voxel.hip (fp64 floor((p - origin) / voxel), origin = min - voxel / 2) -> idx [n,3] int64, or None when
    refused.  floor(x + 1/2) is written floor(x - 1/2) + 1 with x = (p - min) / voxel, which is the same number for every x;
    the defect 'voxel_trunc' truncates towards zero instead, which differs exactly where x - 1/2 is negative."""
    P = f64(P)
    lo = P.min(axis=0)
    if "voxel_trunc" in defects:
        idx = np.trunc((P - lo) / voxel - 0.5).astype(np.int64) + 1
    else:
        idx = np.floor((P - (lo - 0.5 * voxel)) / voxel).astype(np.int64)
    dims = idx.max(axis=0) + 1
    if (dims > voxel_max).any():
        return None
    return idx


def voxel_oracle(P, normals, voxel, idx=None):
    """Means of points (fp32) and normals (fp64) per occupied voxel in ascending key order, from integers (the inputs are
    dyadic: multiples of 2^-11).  idx: the voxel indices to group by (default: the contract's)."""
    q = Q10 / 2
    Pd = f64(P)
    if idx is None:
        idx = np.floor((Pd - (Pd.min(axis=0) - 0.5 * voxel)) / voxel).astype(np.int64)
    dims = idx.max(axis=0) + 1
    key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    Pi, Ni = to_ints(Pd, q), to_ints(normals, q)
    pts, nrm, keys = [], [], sorted(set(key.tolist()))
    for k in keys:
        rows = np.flatnonzero(key == k)
        c = float(len(rows))
        pts.append([np.float32(float(sum(int(v) for v in Pi[rows, a])) * q / c) for a in range(3)])
        nrm.append([float(sum(int(v) for v in Ni[rows, a])) * q / c for a in range(3)])
    return np.array(pts, np.float32), np.array(nrm, np.float64), np.array(keys, np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy model of icp_grid.h and of nb_search_kernel, with seeded defects
# ---------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("radius_le", "radius_fp64", "tie_highest", "cells_26", "no_outside_cells", "narrow_cell", "bucket_twice",
           "cut_ignores_index", "lost_at_second_selection", "max_nn_off_by_one", "voxel_trunc")


class GridModel:
    """The grid of icp_make_grid over the fp32 targets Q for radius r."""

    def __init__(self, Q, r, consts=None, defects=()):
        self.c = consts or source_constants()
        self.defects = frozenset(defects)
        assert self.defects <= set(DEFECTS), self.defects
        Q32 = np.asarray(Q, np.float32)
        self.Q = Q32.astype(np.float64)
        self.nt = len(Q32)
        self.r = r
        self.r2 = r * r if "radius_fp64" in self.defects else radius2(r)
        lo, hi = Q32.min(axis=0).astype(np.float64), Q32.max(axis=0).astype(np.float64)
        ext = hi - lo
        w = r * (0.9 if "narrow_cell" in self.defects else 1.0 + self.c["cell_margin"])
        self.cap_taken = bool(ext.max() / w > self.c["max_cells"])
        if self.cap_taken:
            w = ext.max() / self.c["max_cells"]
        self.lo, self.w = lo, w
        self.n = (np.floor(ext / w) + 1).astype(np.int64)
        h = self.c["hash_min"]
        while h < 2 * self.nt:
            h <<= 1
        self.buckets = h
        tc = np.clip(np.floor((self.Q - lo) / w).astype(np.int64), 0, self.n - 1)
        self.target_cell = tc
        self.target_bucket = self.bucket(tc)

    def bucket(self, cells):
        p = self.c["primes"]
        u = [(cells[..., k].astype(np.uint64) * np.uint64(p[k])) & np.uint64(0xFFFFFFFF) for k in range(3)]
        return ((u[0] ^ u[1] ^ u[2]) & np.uint64(self.buckets - 1)).astype(np.int64)

    def query_buckets(self, P):
        """-> buckets [n,27] (-1: no cell), cells [n,3] as floats (before the range test), any [n]."""
        c = np.floor((P - self.lo) / self.w)
        if "no_outside_cells" in self.defects:
            any_ = ((c >= 0) & (c <= self.n - 1)).all(axis=1)
        else:
            any_ = ((c >= -1) & (c <= self.n)).all(axis=1)
        ci = np.where(any_[:, None], c, 0).astype(np.int64)
        k = np.arange(27)
        off = np.stack([k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1], 1)
        cells = ci[:, None, :] + off[None]
        ok = any_[:, None] & ((cells >= 0) & (cells < self.n)).all(axis=2)
        if "cells_26" in self.defects:
            ok[:, 26] = False
        return np.where(ok, self.bucket(np.where(ok[..., None], cells, 0)), -1), c, any_

    def nearest(self, P):
        """icp_nearest for every row of P (fp64, already transformed) -> corr, d2."""
        qb, _, _ = self.query_buckets(P)
        seen = (self.target_bucket[None, None, :] == qb[:, :, None]).any(axis=1)          # [n, nt]
        d2 = sqdist(P, self.Q)
        ok = seen & ((d2 <= self.r2) if "radius_le" in self.defects else (d2 < self.r2))
        masked = np.where(ok, d2, np.inf)
        if "tie_highest" in self.defects:
            corr = self.nt - 1 - masked[:, ::-1].argmin(axis=1)
        else:
            corr = masked.argmin(axis=1)
        hit = ok.any(axis=1)
        return np.where(hit, corr, -1), np.where(hit, masked[np.arange(len(P)), corr], 0.0)

    def reach(self, P):
        """What the branch-reach test reads: queries in a -1 / n cell, queries with two of their cells in one bucket."""
        qb, c, any_ = self.query_buckets(P)
        outside = any_ & ((c == -1) | (c == self.n)).any(axis=1)
        s = np.sort(qb, axis=1)
        shared = ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)).any(axis=1)
        return {"outside": int(outside.sum()), "shared_bucket": int(shared.sum())}

    def lists(self, max_nn, descending=True):
        """nb_search_kernel for every target as a query of its own cloud: the 27 buckets in lane order (a bucket that two cells
        share once), rounds of `wave` candidates, a selection whenever more than cap - wave wait, one at the end.  The order
        inside a bucket is free on the device; the model takes descending index, so that lower indices arrive late.
        -> idx, d2, count, selections per query."""
        cap, wave = self.c["cap"], self.c["wave"]
        qb, _, _ = self.query_buckets(self.Q)
        by_bucket = {}
        for j in np.argsort(-np.arange(self.nt) if descending else np.arange(self.nt), kind="stable"):
            by_bucket.setdefault(int(self.target_bucket[j]), []).append(int(j))
        by_bucket = {h: np.array(v, np.int64) for h, v in by_bucket.items()}
        keep_nn = max_nn - 1 if "max_nn_off_by_one" in self.defects else max_nn
        idx = np.full((self.nt, max_nn), -1, np.int64)
        out = np.zeros((self.nt, max_nn))
        count = np.zeros(self.nt, np.int64)
        nsel = np.zeros(self.nt, np.int64)
        for i in range(self.nt):
            cd2, cidx = np.zeros(0), np.zeros(0, np.int64)
            thr_d2, thr_idx, selections, since = self.r2, -1, 0, 0

            def select():
                nonlocal cd2, cidx, thr_d2, thr_idx, selections, since
                selections += 1
                if "lost_at_second_selection" in self.defects and selections == 2 and since:
                    cd2, cidx = cd2[:-since], cidx[:-since]
                order = np.lexsort((cidx, cd2))[:keep_nn]
                cd2, cidx = cd2[order], cidx[order]
                since = 0
                if len(cd2) == keep_nn:
                    thr_d2, thr_idx = cd2[-1], cidx[-1]

            visited = set()
            for h in qb[i]:
                h = int(h)
                if h < 0 or (h in visited and "bucket_twice" not in self.defects):
                    continue
                visited.add(h)
                members = by_bucket.get(h, np.zeros(0, np.int64))
                for base in range(0, len(members), wave):
                    m = members[base:base + wave]
                    d = self.Q[i] - self.Q[m]
                    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    if thr_idx < 0:
                        ok = (d2 <= thr_d2) if "radius_le" in self.defects else (d2 < thr_d2)
                    elif "cut_ignores_index" in self.defects:
                        ok = d2 < thr_d2
                    else:
                        ok = (d2 < thr_d2) | ((d2 == thr_d2) & (m < thr_idx))
                    cd2, cidx = np.concatenate([cd2, d2[ok]]), np.concatenate([cidx, m[ok]])
                    since += int(ok.sum())
                    if len(cd2) > cap - wave:
                        select()
            select()
            if "tie_highest" in self.defects:
                order = np.lexsort((-cidx, cd2))
                cd2, cidx = cd2[order], cidx[order]
            k = len(cd2)
            idx[i, :k], out[i, :k], count[i], nsel[i] = cidx, cd2, k, selections
        return idx, out, count, nsel


def ulp_distance_f64(a, b):
    """Distance in units of the last place between two non-negative fp64 numbers."""
    ia = np.array([a], np.float64).view(np.int64)[0]
    ib = np.array([b], np.float64).view(np.int64)[0]
    return abs(int(ia) - int(ib))


def rmse_of(total, n):
    return math.sqrt(total / n) if n else 0.0
