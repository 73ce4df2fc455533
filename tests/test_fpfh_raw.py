"""f-9: FPFH from RAW clouds on the device (pointdsc_amd.features.extract_fpfh_features; csrc/voxel.hip, csrc/fpfh.hip,
csrc/cloud_many.h): the demo's own recipe (demo_registration.py:37-44) -- normals on the raw cloud, open3d's voxel step that also
averages the normals of a voxel, FPFH on the down-sampled cloud with those normals -- and the many-workgroups path of the per-cloud
kernels in front of the descriptor.  DESIGN.md section 8 f-9.

The oracle is the one of tests/test_fpfh.py (imported, not copied) plus an fp64 numpy restatement of the voxel step with normals
below: stable sort by key, sums in input order, VOXEL_NORMAL_RULE (the mean normal is not renormalised unless asked for).  The
fixture tests/golden/demo_raw_crop.npz (tools/make_raw_demo_fixture.py) holds the 6 000 raw vertices nearest the median of each demo
cloud and the oracle's results on them.  As in tests/test_fpfh.py every discrete decision's margin is asserted before anything is
compared, and no point is excused; at the max_nn cut of the RAW stage exact d2 ties are common (the scanner's grid) and allowed,
because the contract breaks them by index.
"""
from __future__ import annotations

import ctypes as C
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
for _p in (ROOT / "tests", ROOT / "tools"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))
from test_fpfh import (FEATURE_MAX_NN, FEATURE_RADIUS, NEAR_TIE, NORMAL_MAX_NN, NORMAL_RADIUS, VOXEL, _cap, _candidates, _dev,  # noqa: E402
                       _nn_rows_fp64, _ulp_diff, fpfh_from_spfh_oracle, neighbours_oracle, normals_oracle, spfh_oracle)

VOXEL_NORMAL_RULE = "sum(n_i) / count, not renormalised"      # open3d 0.9 AccumulatedPoint::GetAverageNormal, restated from memory
CAPACITY_RULE = "more occupied voxels than out_capacity: count -1 and zero rows"
NAMES = ("cloud_bin_0", "cloud_bin_1")
CUT_GAP = 1e-14                                               # about 100 ulp of an fp64 d2: the smallest non-zero relative gap allowed (measured: 3.6e-13)
PATHS = ("one", "many")
REFERENCE_DEMO = Path("/root/reference/demo_data")
# harness.second_view seed of the device_demo_fpfh test, chosen on the CPU: every margin of the second view's oracle is >= NEAR_TIE
# (smallest: radius 1.2e-7) and no nearest-neighbour row of the oracle's descriptors has an fp64 gap below 1e-5 (smallest: 1.3e-4),
# so the excused share is 0 of 100 rows
E2E_SEED = 0


# ---------------------------------------------------------------------------------------------------------------------------
# oracle (fp64 numpy)
# ---------------------------------------------------------------------------------------------------------------------------
def voxel_normals_oracle(points, normals, voxel, renormalize=False):
    """open3d voxel_down_sample of a cloud with normals, as harness.voxel_down_sample restates it for the points: grid anchored at
    min - voxel / 2, stable sort by key, every voxel's points AND normals summed sequentially in input order, divided by the count.
    -> points [m,3] fp32 (the fp64 mean rounded), normals [m,3] fp64 (VOXEL_NORMAL_RULE), counts per voxel [m]."""
    pts = np.asarray(points, np.float32).astype(np.float64)
    nrm = np.asarray(normals, np.float64)
    if len(pts) == 0 or not np.isfinite(pts).all():
        return np.zeros((0, 3), np.float32), np.zeros((0, 3)), np.zeros(0, np.int64)
    origin = pts.min(axis=0) - 0.5 * voxel
    idx = np.floor((pts - origin) / voxel).astype(np.int64)
    dims = idx.max(axis=0) + 1
    key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    order = np.argsort(key, kind="stable")
    key, vals = key[order], np.concatenate([pts, nrm], axis=1)[order]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    cnt = np.diff(np.r_[first, len(key)])
    s = np.zeros((len(first), 6))
    for k in range(int(cnt.max())):                     # sequential, input order: the order is part of the contract
        m = k < cnt
        s = s + np.where(m[:, None], vals[np.where(m, first + k, 0)], 0.0)
    mean = s / cnt[:, None]
    n = mean[:, 3:]
    if renormalize:
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where((length > 0)[:, None], n / length[:, None], n)
    return mean[:, :3].astype(np.float32), n, cnt


def cut_ties_and_gap(P, r, max_nn):
    """At the max_nn cut of every list that is cut: the number of exact d2 ties between the last kept and the first dropped
    entry, and the smallest non-zero gap between them relative to the squared radius (the scale of neighbours_oracle's margins)."""
    r2 = float(np.float32(r * r))
    rows, cols = _candidates(P, r)
    d = P[rows] - P[cols]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    ok = d2 < r2
    rows, cols, d2 = rows[ok], cols[ok], d2[ok]
    order = np.lexsort((cols, d2, rows))
    rows, d2 = rows[order], d2[order]
    total = np.bincount(rows, minlength=len(P))
    pos = np.arange(len(rows)) - (np.cumsum(total) - total)[rows]
    cut = np.flatnonzero(pos == max_nn)
    if not len(cut):
        return 0, math.inf
    gap = (d2[cut] - d2[cut - 1]) / r2
    return int((gap == 0).sum()), float(gap[gap > 0].min()) if (gap > 0).any() else math.inf


def raw_oracle_of(points, voxel=VOXEL, viewpoint=(0.0, 0.0, 0.0)):
    """The demo's recipe on one raw cloud (fp32 points, widened exactly)."""
    P = np.asarray(points, np.float32).astype(np.float64)
    o = {"P": P}
    o["idx_n"], o["d2_n"], o["count_n"], mn = neighbours_oracle(P, 2.0 * voxel, NORMAL_MAX_NN)
    o["normals"], o["gap"], mnorm = normals_oracle(P, o["idx_n"], o["count_n"], viewpoint)
    o["down_points"], o["down_normals"], o["voxel_counts"] = voxel_normals_oracle(points, o["normals"], voxel)
    D = o["down_points"].astype(np.float64)
    o["idx"], o["d2"], o["count"], mf = neighbours_oracle(D, 5.0 * voxel, FEATURE_MAX_NN)
    o["spfh"], ms = spfh_oracle(D, o["down_normals"], o["idx"], o["count"])
    o["fpfh"], o["desc"], _ = fpfh_from_spfh_oracle(o["spfh"], o["idx"], o["d2"], o["count"])
    o["cut_ties"], o["cut_gap"] = cut_ties_and_gap(P, 2.0 * voxel, NORMAL_MAX_NN)
    # the descriptor stage's own cut (max_nn = 100 on the down-sampled cloud) has no ties to allow: it is a margin like the others
    o["margins"] = {"radius_normals": mn["radius"], "radius_fpfh": mf["radius"], "cut_fpfh": mf["cut"], **mnorm, **ms}
    return o


_ORACLE = {}


def fixture():
    if "fixture" not in _ORACLE:
        _ORACLE["fixture"] = dict(np.load(GOLDEN / "demo_raw_crop.npz"))
    return _ORACLE["fixture"]


def raw_oracle(name):
    """The oracle on a crop of the fixture, computed once per session and left unchanged."""
    if name not in _ORACLE:
        _ORACLE[name] = raw_oracle_of(fixture()[f"{name}_points"])
    return _ORACLE[name]


def _assert_margins(name, o):
    print(f"[fpfh-raw] {name}: margins " + " ".join(f"{k}={v:.2e}" for k, v in o["margins"].items())
          + f"  raw cut: {o['cut_ties']} exact ties, smallest non-zero relative gap {o['cut_gap']:.2e}")
    for k, v in o["margins"].items():
        assert v >= NEAR_TIE, (name, k, v)
    assert o["cut_gap"] >= CUT_GAP, (name, o["cut_gap"])


# ---------------------------------------------------------------------------------------------------------------------------
# hand-built voxel edge shapes
# ---------------------------------------------------------------------------------------------------------------------------
def _unit(rs, n):
    v = rs.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def voxel_edge_shapes():
    """name -> (points fp32 [n,3], normals fp64 [n,3]); the cloud with the most voxels comes last (the capacity cases)."""
    rs = np.random.RandomState(5)
    base = np.array([0.3, -0.2, 1.5])
    one_voxel = (base + rs.uniform(0.0, 0.02, (1300, 3))).astype(np.float32)      # within voxel / 2 of the minimum: all in voxel 0
    opp = (base + np.array([[0.0, 0.0, 0.0], [0.01, 0.005, 0.0], [0.2, 0.1, 0.0], [0.21, 0.1, 0.3]])).astype(np.float32)
    n_opp = _unit(rs, 4)
    n_opp[1] = -n_opp[0]                                                            # the first voxel's mean normal is exactly 0
    nan = (base + rs.uniform(0.0, 0.3, (40, 3))).astype(np.float32)
    nan[7, 2] = np.nan
    spread = _cap(700, 0.4, 21)
    return {
        "one_point": (np.array([[0.3, -0.2, 1.5]], np.float32), _unit(rs, 1)),
        "one_voxel_1300": (one_voxel, _unit(rs, 1300)),       # one run across three tiles of 512 (and three workgroups on path many)
        "opposite": (opp, n_opp),
        "nan": (nan, _unit(rs, 40)),
        "spread": (spread, _unit(rs, 700)),
    }


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tests: the fixture, the oracle, the margins, the ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_what_the_oracle_computes(name):
    f, o = fixture(), raw_oracle(name)
    pts = f[f"{name}_points"]
    assert pts.dtype == np.float32 and pts.shape == (6000, 3)
    # discrete results exactly; fp64 results to the rounding of the eigen-solver that produced them (LAPACK builds differ in the
    # last bits: the eigenvector bound 1e-12 / gap of tests/test_fpfh.py, and what it leaves of the features, 1e-9 of their scale 100)
    assert np.array_equal(f[f"{name}_idx"], o["idx_n"]) and np.array_equal(f[f"{name}_count"], o["count_n"])
    assert np.all(np.linalg.norm(f[f"{name}_normals"] - o["normals"], axis=1) <= 1e-12 / o["gap"])
    assert np.array_equal(f[f"{name}_down_points"], o["down_points"])
    assert f[f"{name}_down_normals"].shape == o["down_normals"].shape
    assert np.abs(f[f"{name}_down_normals"] - o["down_normals"]).max() <= 1e-12 / o["gap"].min()
    assert np.abs(f[f"{name}_fpfh"] - o["fpfh"]).max() <= 1e-9 * 100
    assert np.abs(f[f"{name}_desc"] - o["desc"]).max() <= 1e-9
    assert (GOLDEN / "demo_raw_crop.npz").stat().st_size < (1 << 20)


@pytest.mark.skipif(not REFERENCE_DEMO.exists(), reason="the reference's demo clouds are not on this machine")
@pytest.mark.parametrize("name", NAMES)
def test_fixture_crop_is_the_generators(name):
    from make_raw_demo_fixture import reference_crop
    assert np.array_equal(reference_crop(name), fixture()[f"{name}_points"])


@pytest.mark.parametrize("name", NAMES)
def test_voxel_oracle_points_equal_the_harness(name):
    from pointdsc_amd import harness
    o = raw_oracle(name)
    assert np.array_equal(o["down_points"], harness.voxel_down_sample(fixture()[f"{name}_points"], VOXEL))
    assert o["voxel_counts"].sum() == 6000 and len(o["down_points"]) == {"cloud_bin_0": 100, "cloud_bin_1": 149}[name]
    # VOXEL_NORMAL_RULE: a mean of unit normals, shorter than 1 and not renormalised
    length = np.linalg.norm(o["down_normals"], axis=1)
    assert length.max() <= 1.0 + 1e-12 and length.min() > 0.8 and (length < 1.0 - 1e-6).any()
    for shape, (pts, nrm) in voxel_edge_shapes().items():
        got = voxel_normals_oracle(pts, nrm, VOXEL)[0]
        want = harness.voxel_down_sample(pts, VOXEL) if np.isfinite(pts).all() else np.zeros((0, 3), np.float32)
        assert np.array_equal(got, want), shape


@pytest.mark.parametrize("name", NAMES)
def test_margins_on_the_raw_crops(name):
    o = raw_oracle(name)
    assert np.all(o["count_n"] == NORMAL_MAX_NN)                     # every raw point reaches the cut
    assert o["cut_ties"] > 0                                         # ... and exact ties at the cut are part of the input
    _assert_margins(name, o)


def test_header_binding_and_exports_agree_and_arguments_are_checked():
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    from pointdsc_amd import _lib
    arity = {"pdsc_cloud_voxel_workspace_bytes": 2, "pdsc_cloud_voxel_keys": 10, "pdsc_cloud_voxel_means": 15, "pdsc_cloud_neighbours": 13}
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name, na in arity.items():
        m = re.search(rf"\b(?:int|size_t)\s+{name}\s*\(([^)]*)\)", header)
        assert m, name
        assert len(m.group(1).split(",")) == na, name
        assert len(_lib.SIGNATURES[name][1]) == na, name
        assert re.search(rf"\bT {name}\b", out), name
    for rule in ("VOXEL_NORMAL_RULE", "CAPACITY_RULE", "PDSC_PATH_AUTO", "PDSC_PATH_ONE_WORKGROUP", "PDSC_PATH_MANY"):
        assert rule in header, rule
    assert int(re.search(r"#define PDSC_CLOUD_AUTO_MANY (\d+)", header).group(1)) >= 32768
    lib = _lib.load()
    bs, n = 2, 258342
    need = lib.pdsc_cloud_voxel_workspace_bytes(bs, n)
    assert need >= bs * ((n + 511) // 512 + 1) * 4 and lib.pdsc_cloud_voxel_workspace_bytes(0, n) == 0
    assert lib.pdsc_cloud_voxel_workspace_bytes(1, (1 << 24) + 1) == 0
    p, big = C.c_void_p(256), 1 << 40
    keys = lambda **k: lib.pdsc_cloud_voxel_keys(k.get("points", p), None, k.get("voxel", 0.05), p, k.get("ws", p), k.get("wsb", big),  # noqa: E731
                                                 1, 10, k.get("path", 0), None)
    means = lambda **k: lib.pdsc_cloud_voxel_means(p, k.get("normals", p), p, p, p, p, p, k.get("cap", 10), k.get("renorm", 0), p,  # noqa: E731
                                                   k.get("wsb", big), 1, 10, k.get("path", 0), None)
    nbrs = lambda **k: lib.pdsc_cloud_neighbours(p, None, 0.1, 30, k.get("idx", p), p, p, p, k.get("wsb", big), 1, 10,  # noqa: E731
                                                 k.get("path", 0), None)
    # argument validation happens before any HIP call (no GPU here)
    for call, err in ((lambda: keys(points=None), b"null pointer"), (lambda: keys(ws=None), b"null pointer"),
                      (lambda: keys(path=3), b"path"), (lambda: keys(path=-1), b"path"), (lambda: keys(wsb=0), b"workspace"),
                      (lambda: keys(voxel=0.0), b"voxel size"),
                      (lambda: means(normals=None), b"null pointer"), (lambda: means(cap=0), b"out_capacity"),
                      (lambda: means(cap=-5), b"out_capacity"), (lambda: means(path=3), b"path"), (lambda: means(renorm=2), b"renormalize"),
                      (lambda: means(wsb=lib.pdsc_cloud_voxel_workspace_bytes(1, 10) - 1), b"workspace"),
                      (lambda: nbrs(idx=None), b"null pointer"), (lambda: nbrs(path=3), b"path"), (lambda: nbrs(wsb=0), b"workspace")):
        assert call() == -1
        assert err in lib.pdsc_last_error(), (err, lib.pdsc_last_error())


def test_raw_argument_checks_on_cpu():
    import pointdsc_amd
    from pointdsc_amd import extract_fpfh_features, harness, voxel_down_sample_with_normals
    assert {"extract_fpfh_features", "voxel_down_sample_with_normals"} <= set(pointdsc_amd.__all__)
    assert callable(harness.device_demo_fpfh)
    pts, nrm = torch.zeros(1, 10, 3), torch.zeros(1, 10, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        extract_fpfh_features(pts, VOXEL)
    with pytest.raises(RuntimeError, match="GPU"):
        voxel_down_sample_with_normals(pts, nrm, VOXEL)
    with pytest.raises(ValueError, match="path"):
        extract_fpfh_features(pts, VOXEL, path="two")
    with pytest.raises(ValueError, match="capacity"):
        voxel_down_sample_with_normals(pts, nrm, VOXEL, capacity=0)
    with pytest.raises(ValueError, match="voxel_size"):
        extract_fpfh_features(pts, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def _crops():
    return [fixture()[f"{k}_points"] for k in NAMES]


@pytest.mark.gpu
def test_raw_normals_match_the_oracle_on_both_paths():
    from pointdsc_amd import estimate_normals, hybrid_neighbours
    oracles = [raw_oracle(k) for k in NAMES]
    for k, o in zip(NAMES, oracles):
        _assert_margins(k, o)
    pts = [_dev(c) for c in _crops()]
    got = {}
    for path in PATHS:
        nb = hybrid_neighbours(pts, NORMAL_RADIUS, NORMAL_MAX_NN, path=path)
        nrm = estimate_normals(pts, NORMAL_RADIUS, NORMAL_MAX_NN, path=path)
        torch.cuda.synchronize()
        got[path] = (nb, nrm)
        for b, (k, o) in enumerate(zip(NAMES, oracles)):
            assert np.array_equal(nb["count"][b].cpu().numpy(), o["count_n"]), (k, path)
            assert np.array_equal(nb["idx"][b].cpu().numpy(), o["idx_n"]), (k, path)          # exact d2 ties at the cut included
            d2_ulp = float(_ulp_diff(nb["d2"][b].cpu().numpy(), o["d2_n"])[o["d2_n"] > 0].max())
            assert np.all(nb["d2"][b].cpu().numpy()[o["d2_n"] == 0] == 0)
            dn = np.linalg.norm(nrm[b].cpu().numpy() - o["normals"], axis=1)
            print(f"[fpfh-raw] {k} path {path}: d2 ulp {d2_ulp:.2f}  max |dn| gap {float((dn * o['gap']).max()):.3e}")
            assert d2_ulp <= 4, (k, path, d2_ulp)
            assert np.all(dn <= 1e-12 / o["gap"]), (k, path, float((dn * o["gap"]).max()))
    (nb1, n1), (nb2, n2) = got["one"], got["many"]
    for key in ("idx", "d2", "count"):
        assert torch.equal(nb1[key], nb2[key]), key
    assert torch.equal(n1, n2)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_voxel_step_fed_the_oracle_normals_is_bit_equal(path):
    from pointdsc_amd import voxel_down_sample_with_normals
    oracles = [raw_oracle(k) for k in NAMES]
    pts = _dev(np.stack(_crops()))
    nrm = _dev(np.stack([o["normals"] for o in oracles]), np.float64)
    p, n, cnt = voxel_down_sample_with_normals(pts, nrm, VOXEL, path=path)
    pr, nr, cntr = voxel_down_sample_with_normals(pts, nrm, VOXEL, capacity=160, renormalize=True, path=path)
    torch.cuda.synchronize()
    assert cnt.tolist() == cntr.tolist() == [100, 149] and p.shape == (2, 149, 3) and pr.shape == (2, 160, 3)
    for b, (k, o) in enumerate(zip(NAMES, oracles)):
        m = len(o["down_points"])
        assert np.array_equal(p[b, :m].cpu().numpy(), o["down_points"]), k            # the same sums in the same order
        assert np.array_equal(n[b, :m].cpu().numpy(), o["down_normals"]), k
        assert np.array_equal(pr[b, :m].cpu().numpy(), o["down_points"]), k
        want = voxel_normals_oracle(fixture()[f"{k}_points"], o["normals"], VOXEL, renormalize=True)[1]
        ulp = float(_ulp_diff(nr[b, :m].cpu().numpy(), want).max())
        print(f"[fpfh-raw] {k} path {path}: renormalised mean normals within {ulp:.2f} ulp")
        assert ulp <= 2, (k, ulp)
        assert not p[b, m:].any() and not n[b, m:].any() and not pr[b, m:].any() and not nr[b, m:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_voxel_edge_shapes_ragged_batch(path):
    from pointdsc_amd import _lib, voxel_down_sample_with_normals
    from pointdsc_amd.features import PATHS as PATH_CODES
    shapes = voxel_edge_shapes()
    names = list(shapes)
    pts = [_dev(shapes[k][0]) for k in names]
    n_max = max(len(shapes[k][0]) for k in names)
    nrm = torch.zeros(len(names), n_max, 3, dtype=torch.float64, device="cuda:0")
    for b, k in enumerate(names):
        nrm[b, :len(shapes[k][1])] = _dev(shapes[k][1], np.float64)
    want = {r: {k: voxel_normals_oracle(*shapes[k], VOXEL, renormalize=r) for k in names} for r in (False, True)}
    voxels = [len(want[False][k][0]) for k in names]
    assert voxels[0] == 1 and voxels[1] == 1 and voxels[3] == 0 and voxels[4] == max(voxels) > 100
    assert np.all(want[True]["opposite"][1][0] == 0) and np.all(want[False]["opposite"][1][0] == 0)
    cap = max(voxels)                                                 # capacity equal to the largest voxel count
    for renorm in (False, True):
        for capacity in (None, cap):
            p, n, cnt = voxel_down_sample_with_normals(pts, nrm, VOXEL, capacity=capacity, renormalize=renorm, path=path)
            torch.cuda.synchronize()
            assert cnt.tolist() == voxels and p.shape == (len(names), cap, 3) and n.shape == (len(names), cap, 3)
            for b, k in enumerate(names):
                wp, wn, _ = want[renorm][k]
                assert np.array_equal(p[b, :voxels[b]].cpu().numpy(), wp), (k, renorm)
                got_n = n[b, :voxels[b]].cpu().numpy()
                if renorm:
                    live = wn != 0
                    assert np.all(got_n[~live] == 0) and (not live.any() or _ulp_diff(got_n[live], wn[live]).max() <= 2), k
                else:
                    assert np.array_equal(got_n, wn), k
                assert not p[b, voxels[b]:].any() and not n[b, voxels[b]:].any(), k     # padding rows; the NaN cloud: count 0
    # capacity one short of the last cloud's voxel count: count -1 and zero rows, and nothing is written beyond the capacity (the
    # buffers end in one sentinel row, right after the rows of the cloud that does not fit)
    lib, short, bs = _lib.load(), cap - 1, len(names)
    padded = torch.zeros(bs, n_max, 3, device="cuda:0")
    for b, k in enumerate(names):
        padded[b, :len(shapes[k][0])] = pts[b]
    counts_in = torch.tensor([len(shapes[k][0]) for k in names], dtype=torch.int32, device="cuda:0")
    ws = torch.empty(int(lib.pdsc_cloud_voxel_workspace_bytes(bs, n_max)), dtype=torch.uint8, device="cuda:0")
    keys = torch.empty(bs, n_max, dtype=torch.int64, device="cuda:0")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st, code = torch.cuda.current_stream().cuda_stream, PATH_CODES[path]
    assert lib.pdsc_cloud_voxel_keys(ptr(padded), ptr(counts_in), VOXEL, ptr(keys), ptr(ws), ws.numel(), bs, n_max, code, st) == 0
    skeys, perm = torch.sort(keys, dim=1, stable=True)
    out_p = torch.full((bs * short + 1, 3), 7.0, device="cuda:0")
    out_n = torch.full((bs * short + 1, 3), 7.0, dtype=torch.float64, device="cuda:0")
    out_c = torch.full((bs,), 99, dtype=torch.int32, device="cuda:0")
    assert lib.pdsc_cloud_voxel_means(ptr(padded), ptr(nrm), ptr(skeys.contiguous()), ptr(perm.contiguous()), ptr(out_p), ptr(out_n),
                                      ptr(out_c), short, 0, ptr(ws), ws.numel(), bs, n_max, code, st) == 0
    torch.cuda.synchronize()
    assert out_c.tolist() == voxels[:-1] + [-1]
    assert (out_p[-1] == 7.0).all() and (out_n[-1] == 7.0).all()
    assert not out_p[(bs - 1) * short:-1].any() and not out_n[(bs - 1) * short:-1].any()
    for b, k in enumerate(names[:-1]):
        assert np.array_equal(out_p[b * short:b * short + voxels[b]].cpu().numpy(), want[False][k][0]), k
        assert not out_p[b * short + voxels[b]:(b + 1) * short].any(), k
    # a refused call enqueues nothing
    assert lib.pdsc_cloud_voxel_means(ptr(padded), ptr(nrm), ptr(skeys), ptr(perm), ptr(out_p), ptr(out_n), ptr(out_c), 0, 0, ptr(ws),
                                      ws.numel(), bs, n_max, code, st) == -1
    torch.cuda.synchronize()
    assert out_c.tolist() == voxels[:-1] + [-1]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_extract_fpfh_features_matches_the_fixture(path):
    """The tolerances of _compare_stages in tests/test_fpfh.py: fpfh 1e-9 of its scale 100 (1e-7), desc 2 ulp."""
    from pointdsc_amd import extract_fpfh_features
    f = fixture()
    for k in NAMES:
        _assert_margins(k, raw_oracle(k))
    res = extract_fpfh_features([_dev(c) for c in _crops()], VOXEL, path=path)
    torch.cuda.synchronize()
    assert res["counts"].tolist() == [100, 149] and res["desc"].shape == (2, 149, 33)
    for b, k in enumerate(NAMES):
        m = len(f[f"{k}_down_points"])
        assert np.array_equal(res["points"][b, :m].cpu().numpy(), f[f"{k}_down_points"]), k
        dn = float(np.abs(res["normals"][b, :m].cpu().numpy() - f[f"{k}_down_normals"]).max())
        df = float(np.abs(res["fpfh"][b, :m].cpu().numpy() - f[f"{k}_fpfh"]).max())
        du = float(_ulp_diff(res["desc"][b, :m].cpu().numpy(), f[f"{k}_desc"].astype(np.float32)).max())
        print(f"[fpfh-raw] {k} path {path}: max|d fpfh| {df:.3e}  desc ulp {du:.2f}  max|d mean normal| {dn:.3e}")
        assert df <= 1e-9 * 100, (k, df)
        assert du <= 2, (k, du)
        for key in ("points", "normals", "fpfh", "desc"):
            assert not res[key][b, m:].any(), (k, key)


@pytest.mark.gpu
def test_raw_batch_independence_and_graph_replay():
    from pointdsc_amd import extract_fpfh_features
    c0, c1 = _crops()
    x0 = _dev(c0)[None]
    alone = extract_fpfh_features(x0, VOXEL)
    pair = extract_fpfh_features([_dev(c1[:5000]), _dev(c0)], VOXEL)
    run = lambda: extract_fpfh_features(x0, VOXEL, capacity=128)  # noqa: E731  (explicit capacity: no host synchronisation)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        replayed = run()
    g.replay()
    torch.cuda.synchronize()
    m = int(alone["counts"][0])
    assert m == 100 and int(pair["counts"][1]) == m and int(replayed["counts"][0]) == m
    for k in ("points", "normals", "fpfh", "desc"):
        assert torch.equal(alone[k][0, :m], pair[k][1, :m]), k
        assert torch.equal(alone[k][0, :m], replayed[k][0, :m]), k
        assert not replayed[k][0, m:].any(), k
    replayed["desc"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(alone["desc"][0, :m], replayed["desc"][0, :m])


@pytest.mark.gpu
def test_paths_agree_across_the_auto_threshold():
    """70 000 points, above the floor of 32 768 rows that the auto threshold may never go below, on a wide cap whose density keeps
    the lists short (about 45 points within the normal radius).  No oracle at this size: auto, one and many agree bit for bit,
    wherever PDSC_CLOUD_AUTO_MANY stands (2^30 = the many-workgroups path is opt-in, until a raw cloud has been timed)."""
    from pointdsc_amd import extract_fpfh_features
    from pointdsc_amd.features import PATHS as PATH_CODES
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    n = 70000
    assert int(re.search(r"#define PDSC_CLOUD_AUTO_MANY (\d+)", header).group(1)) >= 32768 < n and set(PATH_CODES) == {"auto", "one", "many"}
    pts = _dev(_cap(n, 4.0, 31, R=20.0))[None]
    res = {path: extract_fpfh_features(pts, VOXEL, capacity=32768, path=path) for path in ("auto", "one", "many")}
    torch.cuda.synchronize()
    m = int(res["one"]["counts"][0])
    assert 10000 < m <= 32768
    assert torch.isfinite(res["one"]["desc"]).all() and res["one"]["desc"][0, :m].abs().sum() > 0
    for path in ("auto", "many"):
        for k in ("counts", "points", "normals", "fpfh", "desc"):
            assert torch.equal(res["one"][k], res[path][k]), (path, k)


@pytest.mark.gpu
def test_device_demo_fpfh_registers_like_the_oracle():
    from pointdsc_amd import PointDSC, harness, ops, workloads
    from pointdsc_amd.correspondences import build_correspondences, match_descriptors
    src = fixture()["cloud_bin_0_points"]
    tgt, G, _ = harness.second_view(src, E2E_SEED)
    o_src, o_tgt = raw_oracle("cloud_bin_0"), raw_oracle_of(tgt)
    _assert_margins("second view", o_tgt)
    want_rows, gap = _nn_rows_fp64(o_src["desc"].astype(np.float32), o_tgt["desc"].astype(np.float32))
    close = gap < 1e-5
    assert close.mean() <= 0.005, close.mean()                      # a condition on the input (checked on the CPU for E2E_SEED)
    ps, d_src = harness.device_demo_fpfh(src, VOXEL)
    pt, d_tgt = harness.device_demo_fpfh(tgt, VOXEL)
    assert np.array_equal(ps.cpu().numpy(), o_src["down_points"]) and np.array_equal(pt.cpu().numpy(), o_tgt["down_points"])
    rows = match_descriptors(d_src, d_tgt).cpu().numpy()
    differ = rows != want_rows
    print(f"[fpfh-raw] e2e: {int(differ.sum())} of {len(rows)} nearest-neighbour rows differ, {int(close.sum())} rows have a gap < 1e-5")
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
            print(f"[fpfh-raw] e2e: success {st[0]:.0f} RE {st[1]:.3f} deg TE {st[2]:.3f} cm inlier ratio {st[4]:.3f}")
            outcome.append(bool(st[0] > 0))
    assert outcome[0] == outcome[1]
