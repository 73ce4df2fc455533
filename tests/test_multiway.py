"""f-6: the multiway driver's edge step (pointdsc_amd.multiway; csrc/information.hip, csrc/voxel.hip) against fp64 numpy
restatements of what multiway/test_multi_ate.py does with open3d on the host: get_information_matrix_from_point_clouds and the
overlap gate (:141-149), voxel_down_sample + registration_icp per scale (:54-73).

open3d is not available, so the oracles below ARE the contract.  The correspondence search is the ICP's
(tests/test_icp.py: FLANN_RADIUS_RULE, TIE_RULE, and its oracle, imported from there).  One more detail of open3d cannot be
checked here and is a named rule: IDENTITY_RULE -- open3d 0.9 is believed to start every OpenMP thread's private accumulator of
GetInformationMatrixFromPointClouds from the 6x6 identity (so its result depends on the thread count); later versions start from
zero.  The oracle and the library return the plain sum, which leaves [3][3] = [4][4] = [5][5] = |correspondences| exactly.
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
if str(ROOT / "tests") not in sys.path:
    sys.path.insert(0, str(ROOT / "tests"))
from test_icp import NEAR_TIE, _apply, _evaluate, _is_identity, _perturbed, _three_squares, icp_oracle  # noqa: E402

IDENTITY_RULE = "plain sum (accumulators start from zero)"
EDGE_DISTANCE = 0.05 * 1.4                       # multiway/test_multi_ate.py:60, :144
FIXTURES = ["n1000_s1", "n5000_s5", "kitti_n1500_s4", "lomatch_n10000_s7"]


def _radius(name):
    return 0.6 * 1.4 if name.startswith("kitti") else EDGE_DISTANCE


# ---------------------------------------------------------------------------------------------------------------------------
# oracles (fp64 numpy)
# ---------------------------------------------------------------------------------------------------------------------------
def _rows(Q):
    """The three rows g of every target point: [n,3,6]."""
    x, y, z = Q[:, 0], Q[:, 1], Q[:, 2]
    o, l = np.zeros_like(x), np.ones_like(x)
    return np.stack([np.stack([o, z, -y, l, o, o], 1), np.stack([-z, o, x, o, l, o], 1), np.stack([y, -x, o, o, o, l], 1)], 1)


def information_oracle(S, Q, T, r):
    """open3d GetInformationMatrixFromPointClouds, fp64, IDENTITY_RULE.  S [Ns,3], Q [Nt,3], T [4,4] fp32.
    -> info [6,6], abs_terms [6,6] (the sum of the |terms| of every entry), corr [Ns], margin (smallest relative margin of a
    discrete decision of the correspondence search)."""
    S = np.asarray(S, np.float32).astype(np.float64)
    Q = np.asarray(Q, np.float32).astype(np.float64)
    T = np.asarray(T, np.float32).astype(np.float64)
    if not r > 0:
        return {"info": np.zeros((6, 6)), "abs_terms": np.zeros((6, 6)), "corr": np.full(len(S), -1), "margin": math.inf}
    r2 = float(np.float32(r * r))                       # FLANN_RADIUS_RULE
    P = S.copy() if _is_identity(T) else _apply(T, S)
    corr, _, _, margin = _evaluate(P, Q, r2, r)
    G = _rows(Q[corr[corr >= 0]])
    terms = G[:, :, :, None] * G[:, :, None, :]         # every product rounded on its own, as the kernel's
    return {"info": terms.sum(axis=(0, 1)), "abs_terms": np.abs(terms).sum(axis=(0, 1)), "corr": corr, "margin": margin}


def _skew(q):
    return np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])


def closed_form(Q):
    """sum over q of [[|q|^2 I - q q^T, [q]x], [-[q]x, I]] -- G^T G of G = [-[q]x | I], written out block by block."""
    out = np.zeros((6, 6))
    for q in np.asarray(Q, np.float64):
        out[:3, :3] += q @ q * np.eye(3) - np.outer(q, q)
        out[:3, 3:] += _skew(q)
        out[3:, :3] -= _skew(q)
        out[3:, 3:] += np.eye(3)
    return out


def voxel_oracle(points, voxel):
    """open3d voxel_down_sample as DESIGN.md f-6 states it, one point at a time: -> (means fp32 [m,3] in ascending voxel index,
    the voxel index of every output row)."""
    pts = np.asarray(points, np.float32).astype(np.float64)
    origin = pts.min(axis=0) - 0.5 * voxel
    idx = np.floor((pts - origin) / voxel).astype(np.int64)
    dims = idx.max(axis=0) + 1
    sums, counts = {}, {}
    for p, (ix, iy, iz) in zip(pts, idx):
        k = int((ix * dims[1] + iy) * dims[2] + iz)
        if k in sums:
            sums[k] = sums[k] + p                       # input order
            counts[k] += 1
        else:
            sums[k], counts[k] = p.copy(), 1
    keys = sorted(sums)
    return np.stack([sums[k] / counts[k] for k in keys]).astype(np.float32), np.array(keys, np.int64)


def gate_oracle(info, T32, ns, nt):
    """multiway/test_multi_ate.py:147, negated; T32 is the model's fp32 pose as numpy holds it."""
    return not (info[5, 5] / min(ns, nt) < 0.30 or np.asarray(T32, np.float32).trace() == 4.0)


def box_room(n=60000, seed=11, size=(1.2, 1.0, 0.8)):
    """The seeded dense cloud of the voxel / multi-scale tests: ~n points on the faces of a box room plus 2 mm of noise, so that
    the 0.025 / 0.0125 m scales have something to reduce."""
    from pointdsc_amd import synthetic
    return synthetic.box_room(n, seed=seed, size=size, noise=0.002)


def _multi_scale_case():
    """The pair of the multi-scale ICP test: a 20 000-point room of 0.6 x 0.5 x 0.4 m (as dense as the 60 000-point one) against
    a second view, from 2 deg / 5 cm off.  Every radius test, every nearest-neighbour choice and every convergence test of all three
    scales is a discrete decision, so the oracle's smallest margin shrinks with the number of points; this seed was chosen on
    the CPU among six for the largest one (1.0e-7 on the harness's clouds, 100 x NEAR_TIE; the test asserts it on the device's)."""
    from pointdsc_amd import harness
    src = box_room(20000, size=(0.6, 0.5, 0.4))
    tgt, G, _ = harness.second_view(src, 7)
    return src, tgt, G, _perturbed(G, 2.0, 5.0, 107)


def _fixture(name):
    d = np.load(GOLDEN / f"{name}.npz")
    return d["src_keypts"][0], d["tgt_keypts"][0], d["ref_final_trans"][0]


def _demo_view(seed=0):
    from pointdsc_amd import harness
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    tgt, G, _ = harness.second_view(cloud, seed)
    return cloud, tgt, G.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tests: ABI, exports, argument checks, the oracles against hand-computed cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_multiway_entries_and_library_exports_them():
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    assert re.search(r"\bsize_t\s+pdsc_information_workspace_bytes\s*\(", header)
    for name in ("pdsc_information_matrix", "pdsc_voxel_keys", "pdsc_voxel_means"):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
    assert "IDENTITY_RULE" in header
    from pointdsc_amd import _lib
    names = ("pdsc_information_matrix", "pdsc_information_workspace_bytes", "pdsc_voxel_keys", "pdsc_voxel_means")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name in names:
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\bT {name}\b", out), name
    lib = _lib.load()
    assert lib.pdsc_version() == int(re.search(r"#define\s+PDSC_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    assert lib.pdsc_information_workspace_bytes(2, 5000, 4000) >= 2 * 4000 * 16
    assert lib.pdsc_information_workspace_bytes(0, 10, 10) == 0
    # argument validation happens before any HIP call
    p = C.c_void_p(16)
    assert lib.pdsc_information_matrix(None, None, None, None, None, 0.07, None, None, None, None, 0, 1, 10, 10, None) == -1
    assert b"null pointer" in lib.pdsc_last_error()
    assert lib.pdsc_information_matrix(p, p, p, None, None, 0.07, p, p, None, p, 0, 1, 10, 10, None) == -1
    assert b"workspace" in lib.pdsc_last_error()
    assert lib.pdsc_voxel_keys(p, None, 0.0, p, 1, 10, None) == -1
    assert b"voxel" in lib.pdsc_last_error()
    assert lib.pdsc_voxel_keys(p, None, -0.05, p, 1, 10, None) == -1
    assert lib.pdsc_voxel_keys(None, None, 0.05, p, 1, 10, None) == -1
    assert lib.pdsc_voxel_means(p, p, None, p, p, 1, 10, None) == -1


def test_multiway_module_exports():
    import pointdsc_amd
    from pointdsc_amd import harness, multiway
    for name in ("information_matrix", "voxel_down_sample", "loop_closure_edge", "multi_scale_icp", "local_refinement", "align"):
        assert callable(getattr(multiway, name)), name
        assert getattr(pointdsc_amd, name) is getattr(multiway, name)
        assert name in pointdsc_amd.__all__
    assert callable(harness.multiway_edges) and callable(harness.demo_views)
    assert multiway.EDGE_DISTANCE == 0.05 * 1.4 and multiway.MIN_OVERLAP == 0.30
    assert tuple(multiway.VOXEL_SIZES) == (0.05, 0.025, 0.0125) and tuple(multiway.MAX_ITERS) == (50, 30, 14)


def test_multiway_argument_checks_on_cpu():
    from pointdsc_amd import align, information_matrix, loop_closure_edge, multi_scale_icp, voxel_down_sample
    src, eye = torch.zeros(1, 10, 3), torch.eye(4)[None]
    for call in (lambda: information_matrix(src, src, 0.07, eye), lambda: voxel_down_sample(src, 0.05),
                 lambda: loop_closure_edge(src, src, eye), lambda: multi_scale_icp(src, src, trans=eye),
                 lambda: align(torch.zeros(3, 5), torch.zeros(3, 5))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(ValueError, match=r"\[bs,N,3\]"):
        information_matrix(torch.zeros(1, 10, 2), src, 0.07, eye)
    with pytest.raises(ValueError, match=r"\[bs,N,3\]"):
        voxel_down_sample(torch.zeros(10, 3), 0.05)
    with pytest.raises(ValueError, match="NaN"):
        information_matrix(src, src, float("nan"), eye)
    for bad in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            voxel_down_sample(src, bad)
    with pytest.raises(ValueError, match="voxel_size"):
        multi_scale_icp(src, src, voxel_size=[0.05, 0.0], max_iter=[5, 5], trans=eye)
    with pytest.raises(ValueError, match="scales"):
        multi_scale_icp(src, src, voxel_size=[0.05], max_iter=[5, 5], trans=eye)
    with pytest.raises(ValueError):
        information_matrix([torch.zeros(0, 3)], [torch.zeros(5, 3)], 0.07, eye)


def test_oracle_information_of_four_points_by_hand():
    Q = np.array([[1, 2, 3], [-1, 0, 2], [0.5, -0.5, 0], [10, 10, 10]], np.float32)
    S = Q + np.array([[0.01, 0, 0], [0, -0.02, 0], [0, 0, 0.03], [0.5, 0, 0]], np.float32)       # the fourth is out of reach
    res = information_oracle(S, Q, np.eye(4, dtype=np.float32), 0.07)
    assert list(res["corr"]) == [0, 1, 2, -1]
    # sums over the three matched TARGETS: x 0.5, y 1.5, z 5, xy 1.75, xz 1, yz 6, y2+z2 17.25, x2+z2 15.25, x2+y2 6.5
    by_hand = np.array([[17.25, -1.75, -1.0, 0.0, -5.0, 1.5],
                        [-1.75, 15.25, -6.0, 5.0, 0.0, -0.5],
                        [-1.0, -6.0, 6.5, -1.5, 0.5, 0.0],
                        [0.0, 5.0, -1.5, 3.0, 0.0, 0.0],
                        [-5.0, 0.0, 0.5, 0.0, 3.0, 0.0],
                        [1.5, -0.5, 0.0, 0.0, 0.0, 3.0]])
    np.testing.assert_array_equal(res["info"], by_hand)
    np.testing.assert_array_equal(res["info"], res["info"].T)
    assert res["abs_terms"][0, 1] == 2.25 and res["abs_terms"][3, 3] == 3.0      # |2| + |0| + |-0.25|
    # the pose is applied to the source: moved away by T, nothing matches; moved back onto the targets, the same matrix
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.5, 0, 0]
    assert (information_oracle(S, Q, T, 0.07)["corr"] == -1).all()
    res2 = information_oracle(S - T[:3, 3], Q, T, 0.07)
    np.testing.assert_array_equal(res2["info"], by_hand)


def test_oracle_information_of_exact_copy_is_the_closed_form():
    rs = np.random.RandomState(5)
    Q = rs.uniform(-2, 2, (300, 3)).astype(np.float32)
    res = information_oracle(Q, Q, np.eye(4, dtype=np.float32), 0.07)
    np.testing.assert_array_equal(res["corr"], np.arange(300))
    want = closed_form(Q)
    np.testing.assert_allclose(res["info"], want, rtol=0, atol=300 * 2.0 ** -52 * np.abs(want).max())
    assert res["info"][3, 3] == res["info"][4, 4] == res["info"][5, 5] == 300.0          # IDENTITY_RULE
    # r <= 0: nothing is within reach
    assert not information_oracle(Q, Q, np.eye(4), 0.0)["info"].any()


def test_oracle_information_tie_and_radius_rules():
    eye = np.eye(4, dtype=np.float32)
    # TIE_RULE: the lowest target index among equal distances, reported as a zero-margin decision
    Q = np.array([[0.05, 0, 0], [-0.05, 0, 0], [0, 0.05, 0]], np.float32)
    res = information_oracle(np.zeros((1, 3), np.float32), Q, eye, 0.1)
    assert res["corr"][0] == 0 and res["margin"] == 0.0
    np.testing.assert_array_equal(res["info"], closed_form(Q[:1]))
    # FLANN_RADIUS_RULE: a target whose fp64 squared distance is exactly float32(r r) is excluded by the strict '<'
    r = 0.10
    r2 = float(np.float32(r * r))
    a, b, c = _three_squares(int(r2 * 2.0 ** 30))
    on = (np.array([a, b, c], np.float64) * 2.0 ** -15).astype(np.float32)
    assert float(on[0]) ** 2 + float(on[1]) ** 2 + float(on[2]) ** 2 == r2 < r * r
    res = information_oracle(np.zeros((1, 3), np.float32), on[None], eye, r)
    assert res["corr"][0] == -1 and res["margin"] == 0.0 and not res["info"].any()
    closer = on.copy()
    k = int(np.argmax([a, b, c]))
    closer[k] = np.float32(float(on[k]) - 2.0 ** -15)
    res = information_oracle(np.zeros((1, 3), np.float32), closer[None], eye, r)
    assert res["corr"][0] == 0 and res["info"][5, 5] == 1.0


def test_overlap_gate_truth_table():
    from pointdsc_amd.multiway import overlap_gate
    rot = np.eye(4, dtype=np.float32)
    c, s = np.float32(math.cos(0.3)), np.float32(math.sin(0.3))
    rot[:2, :2] = [[c, -s], [s, c]]
    # fp32 diagonal whose exact sum is not 4 but whose sequential fp32 sum, numpy's trace(), is
    odd = np.diag(np.array([1 - 2.0 ** -24, 1, 1, 1], np.float32))
    assert odd.trace() == 4.0 and odd.astype(np.float64).trace() != 4.0
    cases = [(299.0, 1000, 2000, rot, False),        # 0.299 < 0.30: too small overlapping
             (300.0, 1000, 2000, rot, True),         # 0.30 is not < 0.30
             (300.0, 2000, 1000, rot, True),         # min(Ns, Nt)
             (300.0, 1001, 1001, rot, False),
             (900.0, 1000, 1000, np.eye(4, dtype=np.float32), False),   # trace == 4.0: the model returned the identity
             (900.0, 1000, 1000, odd, False),
             (0.0, 1000, 1000, rot, False)]
    info = np.zeros((len(cases), 6, 6))
    info[:, 5, 5] = [k[0] for k in cases]
    T = np.stack([k[3] for k in cases])
    mins = np.array([min(k[1], k[2]) for k in cases], np.int32)
    keep = overlap_gate(torch.from_numpy(info), torch.from_numpy(T), torch.from_numpy(mins)).numpy()
    assert keep.dtype == np.bool_
    for i, (n55, ns, nt, Ti, want) in enumerate(cases):
        assert gate_oracle(info[i], Ti, ns, nt) == want, i
        assert bool(keep[i]) == want, i


def test_oracle_voxel_means_equal_the_harness_exactly():
    from pointdsc_amd import harness
    cloud = box_room(6000, seed=3)
    for voxel in (0.05, 0.025, 0.0125):
        means, keys = voxel_oracle(cloud, voxel)
        want = harness.voxel_down_sample(cloud, voxel)
        assert means.dtype == want.dtype == np.float32 and means.shape == want.shape
        np.testing.assert_array_equal(means, want)
        assert np.all(np.diff(keys) > 0)
    assert len(harness.voxel_down_sample(cloud, 0.0125)) < len(cloud)


def test_fixtures_have_no_near_tie_in_the_information_search():
    """The GPU comparison below needs every discrete decision of the correspondence search to have a margin: checked here, on
    the CPU, for every case it uses."""
    cases = [(n, *_fixture(n), _radius(n)) for n in FIXTURES]
    S, Q, G = _demo_view(0)
    cases.append(("demo second_view", S, Q, G, EDGE_DISTANCE))
    for name, S, Q, T, r in cases:
        res = information_oracle(S, Q, T, r)
        print(f"[info] {name}: corr {int((res['corr'] >= 0).sum())} / {len(S)} margin {res['margin']:.2e}")
        assert res["margin"] >= NEAR_TIE, (name, res["margin"])
        assert (res["corr"] >= 0).sum() > 0, name


def test_multi_scale_case_has_no_near_tie_on_the_harness_clouds():
    """The chained oracle of the GPU test below, on the harness's down-sampling of the same pair (the device's agrees to 1 ulp):
    the smallest decision margin of every scale, and of the final information matrix, with room above NEAR_TIE."""
    from pointdsc_amd import harness
    from pointdsc_amd.multiway import MAX_ITERS, VOXEL_SIZES
    src, tgt, G, current = _multi_scale_case()
    for voxel, it in zip(VOXEL_SIZES, MAX_ITERS):
        S, Q = harness.voxel_down_sample(src, voxel), harness.voxel_down_sample(tgt, voxel)
        ref = icp_oracle(S, Q, current, r=EDGE_DISTANCE, max_iteration=it)
        print(f"[multi-scale] harness clouds, scale {voxel}: {len(S)} x {len(Q)} iterations {ref['iterations']} margin {ref['margin']:.2e}")
        assert ref["margin"] >= 10 * NEAR_TIE, (voxel, ref["margin"])
        assert 2 <= ref["iterations"] < it
        current = ref["T"].astype(np.float32)
    last = information_oracle(S, Q, current, VOXEL_SIZES[-1] * 1.4)
    assert last["margin"] >= 10 * NEAR_TIE, last["margin"]
    assert len(S) < len(src) and np.abs(current - G).max() < 5e-3


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _gpu_info(S_list, Q_list, T_list, r):
    from pointdsc_amd import information_matrix
    res = information_matrix([_dev(s) for s in S_list], [_dev(q) for q in Q_list], r, _dev(np.stack(T_list)),
                             return_correspondences=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_info(name, S, Q, T, r, info, num, corr=None):
    """One pair's device result against the oracle, with the issue's bounds."""
    ref = information_oracle(S, Q, T, r)
    n = int((ref["corr"] >= 0).sum())
    print(f"[info] {name}: corr {n} / {len(S)} margin {ref['margin']:.2e} max|d| {np.abs(info - ref['info']).max():.3e} "
          f"max bound {(n * 2.0 ** -52 * ref['abs_terms']).max():.3e}")
    assert ref["margin"] >= NEAR_TIE, (name, ref["margin"])
    assert int(num) == n, (name, int(num), n)
    if corr is not None:
        np.testing.assert_array_equal(corr[:len(S)], ref["corr"], err_msg=name)
        assert (corr[len(S):] == -1).all(), name
    assert info[3, 3] == info[4, 4] == info[5, 5] == float(n), name                      # IDENTITY_RULE
    np.testing.assert_array_equal(info, info.T, err_msg=name)
    # reordering an fp64 sum of n terms moves it by at most n 2^-52 sum|terms| (both sums within n 2^-53 of the exact one)
    bound = n * 2.0 ** -52 * ref["abs_terms"]
    assert (np.abs(info - ref["info"]) <= bound).all(), (name, np.abs(info - ref["info"]).max())
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_information_matches_oracle_on_reference_fixtures(name):
    S, Q, T = _fixture(name)
    got = _gpu_info([S], [Q], [T], _radius(name))
    _check_info(name, S, Q, T, _radius(name), got["information"][0], got["num_correspondences"][0], got["correspondences"][0])


@pytest.mark.gpu
def test_information_matches_oracle_on_demo_cloud_second_view():
    S, Q, G = _demo_view(0)
    assert len(S) != len(Q)
    got = _gpu_info([S], [Q], [G], EDGE_DISTANCE)
    ref = _check_info("demo second_view", S, Q, G, EDGE_DISTANCE, got["information"][0], got["num_correspondences"][0],
                      got["correspondences"][0])
    assert (ref["corr"] >= 0).sum() > 0.5 * len(Q)
    # an identity pose is not applied (Eigen isIdentity()): the same as the oracle on the untouched source
    Sg = _apply(G.astype(np.float64), S.astype(np.float64)).astype(np.float32)
    got = _gpu_info([Sg], [Q], [np.eye(4, dtype=np.float32)], EDGE_DISTANCE)
    _check_info("demo, identity pose", Sg, Q, np.eye(4, dtype=np.float32), EDGE_DISTANCE, got["information"][0],
                got["num_correspondences"][0], got["correspondences"][0])


@pytest.mark.gpu
def test_information_ragged_batch_is_bitwise_each_pair_alone():
    cases = [_demo_view(s) for s in range(3)] + [_fixture("n1000_s1")]
    S0, Q0, G0 = cases[0]
    cases.append((S0[:700], Q0[:2500], G0))
    S_list, Q_list, T_list = ([c[k] for c in cases] for k in range(3))
    assert len({len(s) for s in S_list}) > 1 and any(len(s) != len(q) for s, q in zip(S_list, Q_list))
    batch = _gpu_info(S_list, Q_list, T_list, EDGE_DISTANCE)
    for b in range(len(cases)):
        alone = _gpu_info([S_list[b]], [Q_list[b]], [T_list[b]], EDGE_DISTANCE)
        ns = len(S_list[b])
        np.testing.assert_array_equal(batch["information"][b], alone["information"][0], err_msg=f"pair {b}")
        assert batch["num_correspondences"][b] == alone["num_correspondences"][0] > 0
        np.testing.assert_array_equal(batch["correspondences"][b][:ns], alone["correspondences"][0][:ns])
        assert (batch["correspondences"][b][ns:] == -1).all()


@pytest.mark.gpu
def test_information_32_pairs_repeatable_and_graph_capturable():
    from pointdsc_amd import information_matrix
    S, Q, T = _fixture("n5000_s5")
    rs = np.random.RandomState(9)
    Sd, Qd = _dev(np.repeat(S[None], 32, 0)), _dev(np.repeat(Q[None], 32, 0))
    Td = _dev(np.stack([_perturbed(T, 0.2, 0.5, int(s)) for s in rs.randint(0, 10 ** 6, 32)]))
    a = information_matrix(Sd, Qd, EDGE_DISTANCE, Td)
    b = information_matrix(Sd, Qd, EDGE_DISTANCE, Td)
    torch.cuda.synchronize()
    for k in ("information", "num_correspondences"):
        assert torch.equal(a[k], b[k]), k
    assert len(set(a["num_correspondences"].cpu().tolist())) > 1
    # graph capture: one launch, no host synchronisation or allocation inside the library call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        information_matrix(Sd, Qd, EDGE_DISTANCE, Td)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = information_matrix(Sd, Qd, EDGE_DISTANCE, Td)
    g.replay()
    torch.cuda.synchronize()
    for k in ("information", "num_correspondences"):
        assert torch.equal(a[k], c[k]), k
    c["information"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a["information"], c["information"])


@pytest.mark.gpu
def test_information_edge_cases():
    S, Q, G = _demo_view(1)
    bad_T = G.copy()
    bad_T[1, 3] = np.nan
    S_bad = S.copy()
    S_bad[17, 1] = np.inf
    Q_bad = Q.copy()
    Q_bad[5, 0] = np.nan
    got = _gpu_info([S, S_bad, S, S], [Q, Q, Q_bad, Q], [bad_T, G, G, G], EDGE_DISTANCE)
    for b in range(3):
        assert np.isnan(got["information"][b]).all() and got["num_correspondences"][b] == 0, b
        assert (got["correspondences"][b] == -1).all()
    assert np.isfinite(got["information"][3]).all() and got["num_correspondences"][3] > 0
    for r in (0.0, -1.0):
        got = _gpu_info([S], [Q], [G], r)
        assert not got["information"][0].any() and not np.signbit(got["information"][0]).any()
        assert got["num_correspondences"][0] == 0 and (got["correspondences"][0] == -1).all()
    # nothing within reach: the zero matrix
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = 50.0
    got = _gpu_info([S], [Q], [far], EDGE_DISTANCE)
    assert not got["information"][0].any() and got["num_correspondences"][0] == 0


@pytest.mark.gpu
def test_information_duplicate_targets_equal_deduplicated():
    S, Q, G = _demo_view(3)
    rs = np.random.RandomState(5)
    dup = np.concatenate([Q, Q[rs.randint(0, len(Q), 2000)]])
    Qd = dup[rs.permutation(len(dup))]
    _, first = np.unique(Qd, axis=0, return_index=True)
    Qu = Qd[np.sort(first)]                                    # de-duplicated in first-occurrence order
    got = _gpu_info([S, S], [Qd, Qu], [G, G], EDGE_DISTANCE)
    np.testing.assert_array_equal(got["information"][0], got["information"][1])
    assert got["num_correspondences"][0] == got["num_correspondences"][1] > 0
    # the same targets, by coordinates
    c0, c1 = got["correspondences"][0][:len(S)], got["correspondences"][1][:len(S)]
    assert ((c0 >= 0) == (c1 >= 0)).all()
    np.testing.assert_array_equal(Qd[c0[c0 >= 0]], Qu[c1[c1 >= 0]])


def _gpu_voxel(clouds, voxel):
    from pointdsc_amd import voxel_down_sample
    out, counts = voxel_down_sample([_dev(c) for c in clouds], voxel)
    torch.cuda.synchronize()
    assert counts.is_cuda and counts.dtype == torch.int32 and out.shape == (len(clouds), max(len(c) for c in clouds), 3)
    return out.cpu().numpy(), counts.cpu().numpy()


def _ulp_distance(a, b):
    """Distance in units of the last place between fp32 arrays (same-sign or zero values)."""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _check_voxel(name, cloud, voxel, out, count):
    from pointdsc_amd import harness
    want = harness.voxel_down_sample(cloud, voxel)
    assert int(count) == len(want), (name, int(count), len(want))
    got = out[:len(want)]
    assert not out[len(want):].any(), name
    # same voxel order: every output lies in the voxel of the oracle's output of the same row (compared through the means, which
    # agree to 1 ulp, so a permuted order -- different voxels, >= a fraction of a voxel apart -- cannot pass)
    ulp = _ulp_distance(got, want)
    print(f"[voxel] {name} voxel {voxel}: {len(cloud)} -> {len(want)} points, max ulp distance {int(ulp.max())}")
    assert ulp.max() <= 1, (name, int(ulp.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [0.05, 0.025, 0.0125])
def test_voxel_down_sample_matches_harness_on_dense_cloud(voxel):
    cloud = box_room()
    out, counts = _gpu_voxel([cloud], voxel)
    _check_voxel("box room", cloud, voxel, out[0], counts[0])
    assert counts[0] < len(cloud)
    again, counts2 = _gpu_voxel([cloud], voxel)
    np.testing.assert_array_equal(out.view(np.int32), again.view(np.int32))
    np.testing.assert_array_equal(counts, counts2)


@pytest.mark.gpu
def test_voxel_down_sample_ragged_batch_and_edge_cases():
    from pointdsc_amd import harness, voxel_down_sample
    room = box_room(20000, seed=4)
    demo = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    tgt, _, _ = harness.second_view(room, 2)
    one = np.array([[0.3, -0.2, 0.1]], np.float32)
    bad = room[:500].copy()
    bad[7, 2] = np.nan
    clouds = [room, demo, tgt, one, bad, room[:513]]
    out, counts = _gpu_voxel(clouds, 0.025)
    for b, c in enumerate(clouds):
        if b == 4:
            assert counts[b] == 0 and not out[b].any()              # a non-finite point: count 0
            continue
        _check_voxel(f"ragged {b}", c, 0.025, out[b], counts[b])
        alone, n_alone = _gpu_voxel([c], 0.025)
        assert n_alone[0] == counts[b]
        np.testing.assert_array_equal(alone[0][:counts[b]].view(np.int32), out[b][:counts[b]].view(np.int32))
    # a padded tensor with device counts is the same as the list
    padded = np.zeros((len(clouds), len(room), 3), np.float32)
    for b, c in enumerate(clouds):
        padded[b, :len(c)] = c
    out2, counts2 = voxel_down_sample(_dev(padded), 0.025, _dev([len(c) for c in clouds], np.int32))
    np.testing.assert_array_equal(out2.cpu().numpy().view(np.int32), out.view(np.int32))
    np.testing.assert_array_equal(counts2.cpu().numpy(), counts)


def _compare_icp_scale(name, S, Q, init, got, b, max_iteration):
    """tests/test_icp.py's _compare for one scale, with its tolerances.  No near-tie escape: the oracle's smallest decision
    margin on the clouds the device's ICP saw is asserted, so every check below always runs."""
    ref = icp_oracle(S, Q, init, r=EDGE_DISTANCE, max_iteration=max_iteration)
    T32 = got["transformation"][b]
    print(f"[multi-scale] {name}: {len(S)} x {len(Q)} points, iterations {ref['iterations']} (device {int(got['iterations'][b])}) "
          f"corr {int((ref['corr'] >= 0).sum())} rmse {ref['rmse']:.6e} max|dT| {np.abs(T32 - ref['T']).max():.2e} "
          f"margin {ref['margin']:.2e}")
    assert ref["margin"] >= NEAR_TIE, (name, ref["margin"])
    assert int(got["iterations"][b]) == ref["iterations"], (name, int(got["iterations"][b]), ref["iterations"])
    assert int(got["num_correspondences"][b]) == int((ref["corr"] >= 0).sum()), name
    assert float(got["fitness"][b]) == ref["fitness"], name
    assert abs(float(got["inlier_rmse"][b]) - ref["rmse"]) <= 1e-9 * max(ref["rmse"], 1e-300), name
    assert np.abs(T32 - ref["T"]).max() < 1e-6, (name, np.abs(T32 - ref["T"]).max())
    P = _apply(got["transformation_f64"][b], np.asarray(S, np.float32).astype(np.float64))
    corr, _, _, _ = _evaluate(P, np.asarray(Q, np.float32).astype(np.float64), float(np.float32(EDGE_DISTANCE ** 2)), EDGE_DISTANCE)
    np.testing.assert_array_equal(corr, ref["corr"], err_msg=name)
    return ref


@pytest.mark.gpu
def test_multi_scale_icp_matches_chained_oracle_on_dense_cloud():
    from oracle import pointdsc_oracle as O
    from pointdsc_amd import harness, local_refinement, multi_scale_icp
    from pointdsc_amd.multiway import MAX_ITERS, VOXEL_SIZES
    src, tgt, G, init = _multi_scale_case()
    res = multi_scale_icp(_dev(src)[None], _dev(tgt)[None], trans=_dev(init)[None])
    torch.cuda.synchronize()
    assert len(res["scales"]) == 3
    current = init
    counts = []
    for i, sc in enumerate(res["scales"]):
        got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in sc.items()}
        ns, nt = int(got["source_counts"][0]), int(got["target_counts"][0])
        counts.append((ns, nt))
        S, Q = got["source_down"][0][:ns], got["target_down"][0][:nt]
        # the device's clouds are the harness's down-sampling (1 ulp), and the oracle ICP runs on exactly what the device's ICP saw
        want_s = harness.voxel_down_sample(src, VOXEL_SIZES[i])
        assert ns == len(want_s) and _ulp_distance(S, want_s).max() <= 1
        print(f"[multi-scale] scale {VOXEL_SIZES[i]}: device clouds bitwise the harness's: {np.array_equal(S, want_s)}")
        assert nt == len(harness.voxel_down_sample(tgt, VOXEL_SIZES[i]))
        _compare_icp_scale(f"scale {VOXEL_SIZES[i]}", S, Q, current, got, 0, MAX_ITERS[i])
        # the next scale starts from this scale's fp64 pose rounded to fp32
        np.testing.assert_array_equal(got["transformation"][0], got["transformation_f64"][0].astype(np.float32))
        current = got["transformation"][0]
    assert counts[0][0] < counts[1][0] < counts[2][0] < len(src), counts
    # the information matrix of the last scale, at voxel_size[-1] * 1.4
    np.testing.assert_array_equal(res["transformation"].cpu().numpy()[0], current)
    _check_info("last scale", S, Q, current, VOXEL_SIZES[-1] * 1.4, res["information"].cpu().numpy()[0],
                res["num_correspondences"].cpu().numpy()[0])
    re0, te0 = O.registration_errors(torch.from_numpy(init), torch.from_numpy(G.astype(np.float32)))
    re1, te1 = O.registration_errors(torch.from_numpy(current), torch.from_numpy(G.astype(np.float32)))
    print(f"[multi-scale] RE {float(re0):.3f} -> {float(re1):.4f} deg, TE {float(te0):.3f} -> {float(te1):.4f} cm")
    assert re1 < re0 and te1 < te0 and re1 < 0.5 and te1 < 1.0, (re0, te0, re1, te1)
    # local_refinement is the same call with the driver's defaults
    T, info = local_refinement(_dev(src)[None], _dev(tgt)[None], _dev(init)[None])
    assert torch.equal(T, res["transformation"]) and torch.equal(info, res["information"])


@pytest.mark.gpu
def test_loop_closure_edge_gate():
    from pointdsc_amd import loop_closure_edge
    S, Q, G = _demo_view(0)
    S2, Q2, G2 = _demo_view(1)
    # < 30 % overlap: only 15 % of the source has a counterpart in the target
    rs = np.random.RandomState(2)
    S_low = S.copy()
    moved = rs.random_sample(len(S)) < 0.85
    S_low[moved] += 100.0
    # the identity pose on clouds that do overlap under it: dropped by trace == 4.0 alone
    Sg = _apply(G.astype(np.float64), S.astype(np.float64)).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    S_list, Q_list, T_list = [S, S2, S_low, Sg], [Q, Q2, Q, Q], [G, G2, G, eye]
    res = loop_closure_edge([_dev(s) for s in S_list], [_dev(q) for q in Q_list], _dev(np.stack(T_list)))
    torch.cuda.synchronize()
    assert res["keep"].is_cuda and res["keep"].dtype == torch.bool
    keep, info = res["keep"].cpu().numpy(), res["information"].cpu().numpy()
    for b in range(4):
        ref = _check_info(f"gate {b}", S_list[b], Q_list[b], T_list[b], EDGE_DISTANCE, info[b], res["num_correspondences"][b].item())
        assert bool(keep[b]) == gate_oracle(ref["info"], T_list[b], len(S_list[b]), len(Q_list[b])), b
    assert list(keep) == [True, True, False, False]
    assert info[3][5, 5] / min(len(Sg), len(Q)) >= 0.30             # the fourth is dropped by the trace, not by the overlap


@pytest.mark.gpu
def test_align_recovers_the_trajectory_motion():
    from pointdsc_amd import align
    rs = np.random.RandomState(8)
    model = rs.uniform(-2, 2, (3, 40))
    G = _perturbed(np.eye(4), 25.0, 40.0, 3).astype(np.float64)
    data = G[:3, :3] @ model + G[:3, 3:4]
    data[:, 7] += [0.03, 0.0, 0.04]                                 # one fragment 5 cm off
    trans, err = align(model, data)
    assert trans.is_cuda and trans.shape == (4, 4) and err.shape == (40,)
    err = err.cpu().numpy()
    assert np.abs(trans.cpu().numpy() - G).max() < 5e-3
    assert int(np.argmax(err)) == 7 and 4.0 < err[7] < 5.5 and np.median(err) < 0.5


@pytest.mark.gpu
def test_harness_multiway_edges_on_five_views():
    from oracle import pointdsc_oracle as O
    from pointdsc_amd import PointDSC, harness, workloads
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    kw = dict(workloads.BASE_MODEL)
    model = PointDSC(**kw)
    model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    model = model.eval().cuda()
    views = harness.demo_views(cloud, 5)
    edges = harness.multiway_edges(model, views)
    got = {(s, t): (T, info, uncertain) for s, t, T, info, uncertain in edges}
    assert len(got) == len(edges)
    for s in range(4):
        assert (s, s + 1) in got, s                                 # odometry edges are never gated
    assert any(t != s + 1 for s, t in got), "no loop closure survived the overlap gate"
    for (s, t), (T, info, uncertain) in got.items():
        assert uncertain == (t != s + 1), (s, t)
        gt = views[t]["pose"] @ np.linalg.inv(views[s]["pose"])
        re, te = O.registration_errors(torch.from_numpy(T).float(), torch.from_numpy(gt).float())
        print(f"[edges] {s} -> {t}: uncertain {uncertain} RE {float(re):.3f} deg TE {float(te):.3f} cm overlap count {info[5, 5]:.0f}")
        assert re < 15.0 and te < 30.0, (s, t, float(re), float(te))   # the harness's thresholds (eval_scene)
        assert info.shape == (6, 6) and info.dtype == np.float64 and np.array_equal(info, info.T)
        assert info[3, 3] == info[4, 4] == info[5, 5] > 0
        if uncertain:
            assert info[5, 5] / len(views[s]["pts"]) >= 0.30          # one correspondence per source point
