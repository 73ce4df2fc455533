"""f-7: FPFH descriptors on the device (pointdsc_amd.features, csrc/fpfh.hip) against an fp64 numpy restatement of what
misc/cal_fpfh.py:21-26 gets from open3d 0.9 (estimate_normals + compute_fpfh_feature with KDTreeSearchParamHybrid) and of the demo's
normalisation f / (|f|_2 + 1e-6) (demo_registration.py:43).  The algorithm is written out in DESIGN.md section 8 f-7.

open3d is not available, so the oracle below IS the contract.  Three details of open3d are artefacts or cannot be checked here and
are named rules: FLANN_RADIUS_RULE (fp64 d2 < float32(r r), strict), COVARIANCE_ORDER_RULE (the cumulants of a normal are summed in
ascending neighbour index order) and NORMAL_SIGN_RULE (normals point towards a viewpoint, default the origin).  Beside its results
the oracle returns the smallest relative margin of every discrete decision; the tests assert that every margin is >= NEAR_TIE
before they compare anything, and excuse no point as a near-tie.
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

FLANN_RADIUS_RULE = "d2 < float32(r * r)"              # fp64 squared distance against the fp32-rounded squared radius, strict
COVARIANCE_ORDER_RULE = "ascending neighbour index"    # summation order of the nine cumulants
NORMAL_SIGN_RULE = "dot(n, viewpoint - p) >= 0"        # otherwise the normal is negated; the (0, 0, 1) fallback is returned as is
NEAR_TIE = 1e-9                                        # the constant of tests/test_icp.py
VOXEL = 0.05
NORMAL_RADIUS, NORMAL_MAX_NN = 2.0 * VOXEL, 30         # misc/cal_fpfh.py:21-26
FEATURE_RADIUS, FEATURE_MAX_NN = 5.0 * VOXEL, 100
# harness.second_view seed of the end-to-end test, chosen on the CPU: 0.09 % of the oracle's nearest-neighbour rows have an fp64
# gap below 1e-5, and the oracle-fed pipeline run through oracle/pointdsc_oracle.py registers (RE 0.10 deg, TE 0.06 cm)
E2E_SEED = 0

try:
    from scipy.spatial import cKDTree as _KDTree
except ImportError:  # pragma: no cover - brute force below
    _KDTree = None


# ---------------------------------------------------------------------------------------------------------------------------
# oracle (fp64 numpy)
# ---------------------------------------------------------------------------------------------------------------------------
def _candidates(P, r):
    """(row, col) of every pair of points within r (1 + 1e-3): a superset of everything the radius test can accept."""
    rr = r * (1.0 + 1e-3)
    if _KDTree is not None:
        pairs = _KDTree(P).query_pairs(rr, output_type="ndarray")
        self_ = np.arange(len(P), dtype=np.int64)
        return np.r_[pairs[:, 0], pairs[:, 1], self_], np.r_[pairs[:, 1], pairs[:, 0], self_]
    rows, cols = [], []
    for s in range(0, len(P), 256):
        d2 = ((P[s:s + 256, None, :] - P[None, :, :]) ** 2).sum(-1)
        r_, c_ = np.nonzero(d2 < rr * rr)
        rows.append(r_ + s)
        cols.append(c_)
    return np.concatenate(rows), np.concatenate(cols)


def neighbours_oracle(P, r, max_nn):
    """KDTreeFlann::SearchHybrid per point: the at most max_nn nearest points under FLANN_RADIUS_RULE, ascending by (d2, index), the
    point itself included.  P [n,3] fp64.  -> idx [n,max_nn] (-1 beyond the count), d2 [n,max_nn], count [n], margins."""
    n = len(P)
    r2 = float(np.float32(r * r))
    rows, cols = _candidates(P, r)
    d = P[rows] - P[cols]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    margins = {"radius": float(np.abs(d2 - r2).min() / r2)}
    ok = d2 < r2
    rows, cols, d2 = rows[ok], cols[ok], d2[ok]
    order = np.lexsort((cols, d2, rows))
    rows, cols, d2 = rows[order], cols[order], d2[order]
    total = np.bincount(rows, minlength=n)
    start = np.cumsum(total) - total
    pos = np.arange(len(rows)) - start[rows]
    keep = pos < max_nn
    idx = np.full((n, max_nn), -1, dtype=np.int64)
    d2m = np.zeros((n, max_nn))
    idx[rows[keep], pos[keep]] = cols[keep]
    d2m[rows[keep], pos[keep]] = d2[keep]
    cut = np.flatnonzero(pos == max_nn)                 # the first entry that the cut drops, where there is one
    margins["cut"] = float(((d2[cut] - d2[cut - 1]) / r2).min()) if len(cut) else math.inf
    return idx, d2m, np.minimum(total, max_nn), margins


def normals_oracle(P, idx, count, viewpoint=(0.0, 0.0, 0.0)):
    """open3d 0.9 EstimateNormals from the lists (COVARIANCE_ORDER_RULE), then NORMAL_SIGN_RULE.  -> normals [n,3], gap [n]
    (eigen-gap (l1 - l0) / l2; inf for the (0, 0, 1) fallback), margins."""
    n, max_nn = idx.shape
    ids = np.sort(np.where(idx >= 0, idx, np.iinfo(np.int64).max), axis=1)
    s = np.zeros((n, 9))
    for k in range(max_nn):                             # sequential, ascending index: the order is part of the contract
        m = k < count
        q = P[np.where(m, ids[:, k], 0)]
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        term = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1)
        s = s + np.where(m[:, None], term, 0.0)
    cum = s / np.maximum(count, 1)[:, None]
    Cm = np.empty((n, 3, 3))
    Cm[:, 0, 0] = cum[:, 3] - cum[:, 0] * cum[:, 0]
    Cm[:, 0, 1] = Cm[:, 1, 0] = cum[:, 4] - cum[:, 0] * cum[:, 1]
    Cm[:, 0, 2] = Cm[:, 2, 0] = cum[:, 5] - cum[:, 0] * cum[:, 2]
    Cm[:, 1, 1] = cum[:, 6] - cum[:, 1] * cum[:, 1]
    Cm[:, 1, 2] = Cm[:, 2, 1] = cum[:, 7] - cum[:, 1] * cum[:, 2]
    Cm[:, 2, 2] = cum[:, 8] - cum[:, 2] * cum[:, 2]
    w, v = np.linalg.eigh(Cm)
    nv = v[:, :, 0].copy()
    vp = np.asarray(viewpoint, np.float64)
    dot = nv[:, 0] * (vp[0] - P[:, 0]) + nv[:, 1] * (vp[1] - P[:, 1]) + nv[:, 2] * (vp[2] - P[:, 2])
    nv[dot < 0] *= -1.0
    full = count >= 3
    nv[~full] = [0.0, 0.0, 1.0]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(full, (w[:, 1] - w[:, 0]) / w[:, 2], math.inf)
        sign = np.where(full, np.abs(dot) / np.linalg.norm(vp - P, axis=1), math.inf)
    margins = {"eigen_gap": float(gap.min()) if n else math.inf, "sign": float(sign.min()) if n else math.inf}
    return nv, gap, margins


def _bin_margin(t):
    """Distance of the bin coordinate t to the nearest boundary between two bins (1 .. 10; below 0 and above 11 are clamped)."""
    return float(np.abs(t[:, None] - np.arange(1.0, 11.0)[None, :]).min()) if len(t) else math.inf


def spfh_oracle(P, N, idx, count):
    """ComputeSPFHFeature: spfh [n,33], margins."""
    n = len(P)
    k = np.arange(idx.shape[1])[None, :]
    rows, kk = np.nonzero((k >= 1) & (k < count[:, None]))
    cols = idx[rows, kk]
    p1, n1, p2, n2 = P[rows], N[rows], P[cols], N[cols]
    dp = p2 - p1
    d = np.sqrt(dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1] + dp[:, 2] * dp[:, 2])
    dot3 = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        a1 = dot3(n1, dp) / d
        a2 = dot3(n2, dp) / d
        swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
        m1 = np.where(swap[:, None], n2, n1)
        m2 = np.where(swap[:, None], n1, n2)
        dq = np.where(swap[:, None], -dp, dp)
        v = np.stack([dq[:, 1] * m1[:, 2] - dq[:, 2] * m1[:, 1], dq[:, 2] * m1[:, 0] - dq[:, 0] * m1[:, 2],
                      dq[:, 0] * m1[:, 1] - dq[:, 1] * m1[:, 0]], axis=1)
        vn = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        v = v / vn[:, None]
        wv = np.stack([m1[:, 1] * v[:, 2] - m1[:, 2] * v[:, 1], m1[:, 2] * v[:, 0] - m1[:, 0] * v[:, 2],
                       m1[:, 0] * v[:, 1] - m1[:, 1] * v[:, 0]], axis=1)
        f3 = np.where(swap, -a2, a1)
        f2 = dot3(v, m2)
        f1 = np.arctan2(dot3(wv, m2), dot3(m1, m2))
    zero = (d == 0) | (vn == 0)                         # (0, 0, 0), and still binned
    f1, f2, f3 = np.where(zero, 0.0, f1), np.where(zero, 0.0, f2), np.where(zero, 0.0, f3)
    t1, t2, t3 = 11.0 * (f1 + math.pi) / (2.0 * math.pi), 11.0 * (f2 + 1.0) * 0.5, 11.0 * (f3 + 1.0) * 0.5
    hist = np.zeros((n, 33))
    for off, t in ((0, t1), (11, t2), (22, t3)):
        np.add.at(hist, (rows, off + np.clip(np.floor(t), 0, 10).astype(np.int64)), 1.0)
    spfh = hist * np.where(count > 1, 100.0 / np.maximum(count - 1, 1), 0.0)[:, None]
    same = np.all(n1 == n2, axis=1) | np.all(n1 == -n2, axis=1)       # bit-equal normals up to sign: an exact tie on both sides
    live = d != 0
    sw = live & ~same
    margins = {"swap": float(np.abs(np.abs(a1[sw]) - np.abs(a2[sw])).min()) if sw.any() else math.inf,
               "vnorm": float((vn[live] / d[live]).min()) if live.any() else math.inf,
               "bins": min(_bin_margin(t1), _bin_margin(t2), _bin_margin(t3))}
    return spfh, margins


def fpfh_from_spfh_oracle(spfh, idx, d2, count):
    """ComputeFPFHFeature: fpfh [n,33] fp64 and the demo's fp64 f / (|f|_2 + 1e-6)."""
    n, max_nn = idx.shape
    f = np.zeros((n, 33))
    ssum = np.zeros((n, 3))
    for k in range(1, max_nn):                          # list order; a block's sum runs neighbour-major, bin-minor
        m = (k < count) & (d2[:, k] != 0)
        if not m.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            val = np.where(m[:, None], spfh[np.where(m, idx[:, k], 0)] / d2[:, k][:, None], 0.0)
        f = f + val
        for j in range(33):
            ssum[:, j // 11] = ssum[:, j // 11] + val[:, j]
    with np.errstate(divide="ignore"):
        scale = np.where(ssum != 0, 100.0 / ssum, 0.0)
    f = f * np.repeat(scale, 11, axis=1) + spfh
    desc = f / (np.sqrt((f * f).sum(axis=1)) + 1e-6)[:, None]
    return f, desc, ssum


def fpfh_oracle(points, voxel=VOXEL, viewpoint=(0.0, 0.0, 0.0)):
    """The whole recipe on one cloud (fp32 points, widened exactly)."""
    P = np.asarray(points, np.float32).astype(np.float64)
    out = {"P": P}
    out["idx_n"], _, out["count_n"], mn = neighbours_oracle(P, 2.0 * voxel, NORMAL_MAX_NN)
    out["normals"], out["gap"], mnorm = normals_oracle(P, out["idx_n"], out["count_n"], viewpoint)
    out["idx"], out["d2"], out["count"], mf = neighbours_oracle(P, 5.0 * voxel, FEATURE_MAX_NN)
    out["spfh"], ms = spfh_oracle(P, out["normals"], out["idx"], out["count"])
    out["fpfh"], out["desc"], out["block_sum"] = fpfh_from_spfh_oracle(out["spfh"], out["idx"], out["d2"], out["count"])
    out["margins"] = {"radius_normals": mn["radius"], "cut_normals": mn["cut"], "radius_fpfh": mf["radius"], "cut_fpfh": mf["cut"],
                      **mnorm, **ms}
    return out


_DEMO = {}


def demo_oracle(name):
    """The oracle on a demo cloud, computed once per session and left unchanged."""
    if name not in _DEMO:
        _DEMO[name] = fpfh_oracle(np.load(GOLDEN / "demo_clouds_vox005.npz")[name])
    return _DEMO[name]


def _assert_margins(name, margins):
    print(f"[fpfh] {name}: margins " + " ".join(f"{k}={v:.2e}" for k, v in margins.items()))
    for k, v in margins.items():
        assert v >= NEAR_TIE, (name, k, v)


# ---------------------------------------------------------------------------------------------------------------------------
# hand-built edge shapes: a noisy sphere cap (never an exact plane: there a1 ~ a2 ~ 0 and the swap is a near-tie by construction)
# ---------------------------------------------------------------------------------------------------------------------------
def _cap(n, rho, seed, centre=(0.3, -0.2, 1.5), R=1.0, sigma=0.002):
    """n points of a sphere cap of radius R (disc radius rho around its pole), noise sigma, fp32."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(0, 2 * math.pi, n)
    rad = rho * np.sqrt(rs.uniform(0, 1, n))
    u, v = rad * np.cos(a), rad * np.sin(a)
    pts = np.stack([u, v, np.sqrt(R * R - u * u - v * v) - R], axis=1) + rs.standard_normal((n, 3)) * sigma
    return (pts + np.asarray(centre)).astype(np.float32)


def edge_shapes():
    twin = _cap(25, 0.09, 14)                            # fewer than 30 points: the twins cannot straddle a cut
    twin[24] = twin[5]                                   # one exact duplicate pair: 5 and 24
    line = (np.array([[0.3, -0.2, 1.5]]) + np.arange(3)[:, None] * 0.15 * np.array([[0.6, 0.64, 0.48]])).astype(np.float32)
    return {
        "n1": np.array([[0.3, -0.2, 1.5]], np.float32),
        "n2": np.array([[0.3, -0.2, 1.5], [0.34, -0.17, 1.52]], np.float32),
        "n3_collinear": line,                            # spacing 0.15 > the normal radius: (0, 0, 1) fallback normals
        "n70": _cap(70, 0.11, 11),                       # count < max_nn, straddling a 64-lane boundary
        "n150": _cap(150, 0.115, 12),                    # the max_nn = 100 cut with more than 128 candidates
        "twin": twin,
    }


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tests: the oracle itself, the margins of the fixture, the ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cloud_bin_0", "cloud_bin_1"])
def test_oracle_self_checks_and_margins_on_demo_cloud(name):
    import pointdsc_amd.features as F
    assert (F.NORMAL_RADIUS_VOXELS * VOXEL, F.NORMAL_MAX_NN, F.FEATURE_RADIUS_VOXELS * VOXEL, F.FEATURE_MAX_NN) == \
        (NORMAL_RADIUS, NORMAL_MAX_NN, FEATURE_RADIUS, FEATURE_MAX_NN)
    o = demo_oracle(name)
    P, n = o["P"], len(o["P"])
    # lists: the point itself (or a lower-index duplicate) first, ascending distances, the cut is part of the hot path
    assert np.all(o["d2"][:, 0] == 0) and np.all(o["idx"][:, 0] <= np.arange(n))
    assert (o["count"] == FEATURE_MAX_NN).mean() > 0.5
    # every SPFH block of a point with count > 1 sums to 100
    blocks = o["spfh"].reshape(n, 3, 11).sum(axis=2)
    many = o["count"] > 1
    assert many.any() and np.abs(blocks[many] - 100.0).max() < 1e-9
    assert np.all(blocks[~many] == 0)
    # every FPFH block sums to 200 where the weighted sum is not 0
    fb = o["fpfh"].reshape(n, 3, 11).sum(axis=2)
    live = o["block_sum"] != 0
    assert live.any() and np.abs(fb[live] - 200.0).max() < 1e-9
    # unit normals that satisfy the sign rule
    assert np.abs(np.linalg.norm(o["normals"], axis=1) - 1.0).max() < 1e-12
    full = o["count_n"] >= 3
    assert np.all((o["normals"][full] * (0.0 - P[full])).sum(axis=1) >= 0)
    # the demo's normalisation
    assert np.abs(np.linalg.norm(o["desc"], axis=1) - 1.0).max() < 1e-6
    _assert_margins(name, o["margins"])


def test_oracle_on_edge_shapes():
    shapes = edge_shapes()
    o = {k: fpfh_oracle(v) for k, v in shapes.items()}
    for k, v in o.items():
        _assert_margins(k, v["margins"])
    assert np.all(o["n1"]["fpfh"] == 0) and np.all(o["n1"]["desc"] == 0) and o["n1"]["normals"].tolist() == [[0.0, 0.0, 1.0]]
    assert o["n2"]["count"].tolist() == [2, 2] and o["n2"]["normals"].tolist() == [[0.0, 0.0, 1.0]] * 2
    assert o["n3_collinear"]["count_n"].tolist() == [1, 1, 1] and o["n3_collinear"]["count"].tolist() == [2, 3, 2]
    assert np.all(o["n70"]["count"] == 70)
    assert np.all(o["n150"]["count"] == 100)
    t = o["twin"]
    # the higher-index twin finds its twin first and itself second, both at distance 0; the pair is binned as (0, 0, 0) in
    # SPFH (bins 5, 16, 27) and skipped in FPFH
    assert t["idx"][24, :2].tolist() == [5, 24] and t["idx"][5, :2].tolist() == [5, 24] and np.all(t["d2"][[5, 24], :2] == 0)
    assert np.array_equal(t["normals"][5], t["normals"][24])
    assert np.array_equal(t["fpfh"][5], t["fpfh"][24]) and np.isfinite(t["fpfh"]).all()
    assert np.all(t["spfh"][5, [5, 16, 27]] >= 100.0 / 24 - 1e-12)


def test_header_declares_fpfh_and_library_exports_it():
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    from pointdsc_amd import _lib
    arity = {"pdsc_hybrid_neighbours_workspace_bytes": 2, "pdsc_hybrid_neighbours": 12, "pdsc_estimate_normals": 10, "pdsc_spfh": 10,
             "pdsc_fpfh_from_spfh": 11, "pdsc_fpfh_workspace_bytes": 4, "pdsc_fpfh": 15}
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name, na in arity.items():
        m = re.search(rf"\b(?:int|size_t)\s+{name}\s*\(([^)]*)\)", header)
        assert m, name
        assert len(m.group(1).split(",")) == na, name
        assert len(_lib.SIGNATURES[name][1]) == na, name
        assert re.search(rf"\bT {name}\b", out), name
    for rule in ("FLANN_RADIUS_RULE", "COVARIANCE_ORDER_RULE", "NORMAL_SIGN_RULE"):
        assert rule in header, rule
    lib = _lib.load()
    assert lib.pdsc_version() == int(re.search(r"#define\s+PDSC_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    n, bs = 5333, 2
    assert lib.pdsc_fpfh_workspace_bytes(bs, n, 30, 100) >= bs * n * (30 * 4 + 100 * 12 + 33 * 8 + 16)
    assert lib.pdsc_hybrid_neighbours_workspace_bytes(bs, n) >= bs * n * 16
    assert lib.pdsc_fpfh_workspace_bytes(0, n, 30, 100) == 0 and lib.pdsc_fpfh_workspace_bytes(1, n, 30, 129) == 0
    # argument validation happens before any HIP call
    p = C.c_void_p(256)
    assert lib.pdsc_fpfh(None, None, 0.1, 30, 0.25, 100, None, p, p, None, p, 1 << 40, 1, 10, None) == -1
    assert b"null pointer" in lib.pdsc_last_error()
    assert lib.pdsc_fpfh(p, None, 0.1, 30, 0.25, 129, None, p, p, None, p, 1 << 40, 1, 10, None) == -1
    assert b"max_nn" in lib.pdsc_last_error()
    assert lib.pdsc_fpfh(p, None, 0.0, 30, 0.25, 100, None, p, p, None, p, 1 << 40, 1, 10, None) == -1
    assert b"radii" in lib.pdsc_last_error()
    assert lib.pdsc_fpfh(p, None, 0.1, 30, 0.25, 100, None, p, p, None, p, 0, 1, 10, None) == -1
    assert b"workspace" in lib.pdsc_last_error()
    assert lib.pdsc_hybrid_neighbours(p, None, -1.0, 100, p, p, p, p, 1 << 40, 1, 10, None) == -1
    assert lib.pdsc_hybrid_neighbours(p, None, 0.25, 0, p, p, p, p, 1 << 40, 1, 10, None) == -1
    assert lib.pdsc_estimate_normals(p, None, None, p, 30, None, p, 1, 10, None) == -1
    assert lib.pdsc_spfh(p, None, p, p, p, 200, p, 1, 10, None) == -1
    assert lib.pdsc_fpfh_from_spfh(p, None, p, p, p, 100, None, None, 1, 10, None) == -1


def test_fpfh_argument_checks_on_cpu():
    import pointdsc_amd
    from pointdsc_amd import compute_fpfh_feature, estimate_normals, fpfh_descriptors, hybrid_neighbours
    assert pointdsc_amd.features.FPFH_DIM == 33
    pts = torch.zeros(1, 10, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        fpfh_descriptors(pts, VOXEL)
    with pytest.raises(ValueError, match="max_nn"):
        hybrid_neighbours(pts, 0.25, 129)
    with pytest.raises(ValueError, match="radius"):
        estimate_normals(pts, 0.0)
    with pytest.raises(ValueError, match="viewpoint"):
        estimate_normals(pts, 0.1, viewpoint=[0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match=r"\[bs,N,3\]"):
        compute_fpfh_feature(torch.zeros(10, 3), 0.25, normal_radius=0.1)
    with pytest.raises(ValueError, match="normal_radius"):
        compute_fpfh_feature(pts, 0.25)
    from pointdsc_amd import harness
    cloud = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="descriptor"):
        next(iter(harness.demo_pairs(cloud, 1, descriptor="fcgf")))
    with pytest.raises(ValueError, match="descriptor"):
        harness.demo_views(cloud, 2, descriptor="fcgf")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _ulp_diff(a, b):
    """|a - b| in units in the last place of b (same dtype, finite)."""
    return np.abs(a - b) / np.spacing(np.abs(b).astype(b.dtype))


def _compare_stages(name, cloud, o, nb_n, normals, nb, feat, whole, b):
    """Cloud b of a batch, stage by stage and whole, against its oracle; -> the measured maxima."""
    n = len(cloud)
    cnt = o["count"]
    live = np.arange(FEATURE_MAX_NN)[None, :] < cnt[:, None]
    # a. lists: indices and counts exactly, distances within 4 ulp
    assert np.array_equal(nb_n["count"][b, :n], o["count_n"]), name
    assert np.array_equal(nb_n["idx"][b, :n], o["idx_n"]), name
    assert np.array_equal(nb["count"][b, :n], cnt), name
    assert np.array_equal(nb["idx"][b, :n], o["idx"]), name
    assert np.all(nb["d2"][b, :n][~live] == 0)
    d2_ulp = float(_ulp_diff(nb["d2"][b, :n][live], o["d2"][live]).max())
    assert d2_ulp <= 4, (name, d2_ulp)
    # b. normals within 1e-12 / eigen-gap (eigenvector perturbation bound; the fallback has gap inf: exact)
    dn = np.linalg.norm(normals[b, :n] - o["normals"], axis=1)
    assert np.all(dn <= 1e-12 / o["gap"]), (name, float((dn * o["gap"]).max()))
    # c + d. through the stage entries (device normals) and through pdsc_fpfh
    res = {"d2_ulp": d2_ulp, "normal_x_gap": float(np.where(np.isfinite(o["gap"]), dn * o["gap"], 0.0).max())}
    assert np.abs(feat["spfh"][b, :n] - o["spfh"]).max() <= 1e-9 * 100, (name, np.abs(feat["spfh"][b, :n] - o["spfh"]).max())
    want32 = o["desc"].astype(np.float32)
    for tag, r in (("stages", feat), ("whole", whole)):
        df = float(np.abs(r["fpfh"][b, :n] - o["fpfh"]).max())
        du = float(_ulp_diff(r["desc"][b, :n], want32).max())
        print(f"[fpfh] {name} {tag}: max|d fpfh| {df:.3e}  desc ulp {du:.2f}  d2 ulp {d2_ulp:.2f}  max |dn| gap {res['normal_x_gap']:.3e}")
        assert df <= 1e-9 * 100, (name, tag, df)
        assert du <= 2, (name, tag, du)
        res[tag + "_fpfh"], res[tag + "_desc_ulp"] = df, du
    assert np.array_equal(whole["normals"][b, :n], normals[b, :n]), name
    # padding rows are zero
    for arr in (nb["count"][b, n:], normals[b, n:], whole["fpfh"][b, n:], whole["desc"][b, n:], feat["fpfh"][b, n:]):
        assert not np.any(arr), name
    return res


def _gpu_all(clouds):
    """Every stage through its own entry, then pdsc_fpfh whole, on a ragged batch -> numpy results."""
    from pointdsc_amd import compute_fpfh_feature, estimate_normals, hybrid_neighbours
    pts = [_dev(c) for c in clouds]
    nb_n = hybrid_neighbours(pts, NORMAL_RADIUS, NORMAL_MAX_NN)
    normals = estimate_normals(pts, NORMAL_RADIUS, NORMAL_MAX_NN)
    nb = hybrid_neighbours(pts, FEATURE_RADIUS, FEATURE_MAX_NN)
    feat = compute_fpfh_feature(pts, FEATURE_RADIUS, FEATURE_MAX_NN, normals=normals)
    whole = compute_fpfh_feature(pts, FEATURE_RADIUS, FEATURE_MAX_NN, normal_radius=NORMAL_RADIUS, normal_max_nn=NORMAL_MAX_NN)
    torch.cuda.synchronize()
    cpu = lambda d: {k: v.cpu().numpy() for k, v in d.items()}  # noqa: E731
    return cpu(nb_n), normals.cpu().numpy(), cpu(nb), cpu(feat), cpu(whole)


@pytest.mark.gpu
def test_fpfh_edge_shapes_ragged_batch():
    shapes = edge_shapes()
    oracles = {k: fpfh_oracle(v) for k, v in shapes.items()}
    for k, o in oracles.items():
        _assert_margins(k, o["margins"])
    names = list(shapes)
    got = _gpu_all([shapes[k] for k in names])                       # one ragged batch: 1 .. 150 points, padded to 150
    for b, k in enumerate(names):
        _compare_stages(k, shapes[k], oracles[k], *got, b)
    whole = got[4]
    assert not np.any(whole["fpfh"][0, 0]) and not np.any(whole["desc"][0, 0]) and whole["normals"][0, 0].tolist() == [0.0, 0.0, 1.0]
    t = names.index("twin")
    assert got[2]["idx"][t, 24, :2].tolist() == [5, 24] and np.all(got[2]["d2"][t, 24, :2] == 0)
    assert np.array_equal(whole["fpfh"][t, 5], whole["fpfh"][t, 24])


@pytest.mark.gpu
def test_fpfh_demo_clouds_ragged_batch():
    names = ["cloud_bin_0", "cloud_bin_1"]
    d = np.load(GOLDEN / "demo_clouds_vox005.npz")
    oracles = [demo_oracle(k) for k in names]
    for k, o in zip(names, oracles):
        _assert_margins(k, o["margins"])
    got = _gpu_all([d[k] for k in names])
    for b, k in enumerate(names):
        _compare_stages(k, d[k], oracles[b], *got, b)


@pytest.mark.gpu
def test_fpfh_batch_independence_and_graph_replay():
    from pointdsc_amd import compute_fpfh_feature
    d = np.load(GOLDEN / "demo_clouds_vox005.npz")
    c0, c1 = d["cloud_bin_0"], d["cloud_bin_1"]
    n0 = len(c0)
    run = lambda p: compute_fpfh_feature(p, FEATURE_RADIUS, FEATURE_MAX_NN, normal_radius=NORMAL_RADIUS)  # noqa: E731
    x0 = _dev(c0)[None]
    alone = run(x0)
    pair = run([_dev(c1), _dev(c0)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x0)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        replayed = run(x0)
    g.replay()
    torch.cuda.synchronize()
    for k in ("fpfh", "desc", "normals"):
        assert torch.equal(alone[k][0], pair[k][1, :n0]), k
        assert torch.equal(alone[k], replayed[k]), k
    replayed["desc"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(alone["desc"], replayed["desc"])


@pytest.mark.gpu
def test_fpfh_nan_cloud_and_rejected_arguments():
    from pointdsc_amd import _lib, compute_fpfh_feature, hybrid_neighbours
    shapes = edge_shapes()
    good, bad = shapes["n70"], shapes["n150"].copy()
    bad[17, 1] = np.nan
    res = compute_fpfh_feature([_dev(bad), _dev(good)], FEATURE_RADIUS, FEATURE_MAX_NN, normal_radius=NORMAL_RADIUS)
    nb = hybrid_neighbours([_dev(bad), _dev(good)], FEATURE_RADIUS, FEATURE_MAX_NN)
    alone = compute_fpfh_feature(_dev(good)[None], FEATURE_RADIUS, FEATURE_MAX_NN, normal_radius=NORMAL_RADIUS)
    torch.cuda.synchronize()
    for k in ("fpfh", "desc", "normals"):
        assert torch.isnan(res[k][0]).all(), k                     # NaN rows for that cloud only
        assert torch.equal(res[k][1, :70], alone[k][0]), k
        assert not res[k][1, 70:].any(), k
    assert (nb["count"][0] == -1).all() and (nb["count"][1, :70] == 70).all() and (nb["count"][1, 70:] == 0).all()
    # rejected before anything is enqueued
    lib = _lib.load()
    pts = _dev(good)[None]
    ws = torch.empty(int(lib.pdsc_fpfh_workspace_bytes(1, 70, 30, 100)), dtype=torch.uint8, device="cuda:0")
    out = torch.full((1, 70, 33), 7.0, dtype=torch.float32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    call = lambda points, rn, nn: lib.pdsc_fpfh(points, None, rn, 30, FEATURE_RADIUS, nn, None, None, p(out), None, p(ws),  # noqa: E731
                                                ws.numel(), 1, 70, st)
    assert call(p(pts), NORMAL_RADIUS, 129) == -1
    assert call(p(pts), 0.0, 100) == -1 and call(p(pts), -1.0, 100) == -1
    assert call(None, NORMAL_RADIUS, 100) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call(p(pts), NORMAL_RADIUS, 100) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, alone["desc"])


def _nn_rows_fp64(src_desc, tgt_desc):
    """Nearest target row per source row and the best-versus-second-best gap of the fp64 distances sqrt(2 - 2 s.t + 1e-6)."""
    s, t = src_desc.astype(np.float64), tgt_desc.astype(np.float64)
    dist = np.sqrt(np.maximum(2.0 - 2.0 * (s @ t.T) + 1e-6, 0.0))
    two = np.partition(dist, 1, axis=1)[:, :2]
    return dist.argmin(axis=1), two[:, 1] - two[:, 0]


@pytest.mark.gpu
def test_fpfh_end_to_end_registration_matches_oracle_descriptors():
    from pointdsc_amd import PointDSC, fpfh_descriptors, harness, ops, workloads
    from pointdsc_amd.correspondences import build_correspondences, match_descriptors
    src = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    tgt, G, _ = harness.second_view(src, E2E_SEED)
    o_src, o_tgt = demo_oracle("cloud_bin_0"), fpfh_oracle(tgt)
    _assert_margins("second view", o_tgt["margins"])
    want_rows, gap = _nn_rows_fp64(o_src["desc"].astype(np.float32), o_tgt["desc"].astype(np.float32))
    close = gap < 1e-5
    assert close.mean() < 0.005, close.mean()                       # a condition on the input (checked on the CPU for E2E_SEED)
    ps, pt = _dev(src), _dev(tgt)
    d_src, d_tgt = fpfh_descriptors(ps[None], VOXEL)[0], fpfh_descriptors(pt[None], VOXEL)[0]
    rows = match_descriptors(d_src, d_tgt).cpu().numpy()
    differ = rows != want_rows
    print(f"[fpfh] e2e: {int(differ.sum())} of {len(rows)} nearest-neighbour rows differ, {int(close.sum())} rows have a gap < 1e-5")
    assert not np.any(differ & ~close)
    kw = dict(workloads.BASE_MODEL)
    model = PointDSC(**kw)
    model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    model = model.eval().cuda()
    outcome = []
    with torch.no_grad():
        for a, b in ((d_src, d_tgt), (_dev(o_src["desc"]), _dev(o_tgt["desc"]))):
            c = build_correspondences(a, b, ps, pt)
            res = model({"corr_pos": c["corr_pos"], "src_keypts": c["src_keypts"], "tgt_keypts": c["tgt_keypts"], "testing": True})
            gt = _dev(G)
            labels = harness.gt_labels_from_trans(c["src_keypts"][0], c["tgt_keypts"][0], gt, kw["inlier_threshold"])[None]
            st = ops.eval_stats(res["final_trans"], gt[None], res["final_labels"], labels)[0].cpu().numpy()
            print(f"[fpfh] e2e: success {st[0]:.0f} RE {st[1]:.3f} deg TE {st[2]:.3f} cm inlier ratio {st[4]:.3f}")
            outcome.append(bool(st[0] > 0))
    assert outcome[0] == outcome[1]
    # the harness's descriptor="fpfh" path is this pipeline
    row = harness.eval_scene(model, harness.demo_pairs(src, 1, seed=E2E_SEED, descriptor="fpfh", voxel=VOXEL))[0]
    assert bool(row[0] > 0) == outcome[0]
