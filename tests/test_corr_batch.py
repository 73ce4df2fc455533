"""Correspondence construction for a batch of pairs over a pool of clouds (pointdsc_amd.correspondences.build_correspondences_batch,
csrc/match_batch.hip, include/pointdsc_hip.h "f-19").  CPU part: symbols, argument checks, the batch oracle (tests/corr_batch_oracle.py)
on a hand-worked case, the fp64 label rule at its threshold.  GPU part: every pair of a batch bit for bit against the per-pair entry
points, independence of the target split, ties / NaN inside a batch, labels against the fp64 oracle, repeatability without a host
read, and the batched callers of the harness against their one-pair-per-call forms."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_batch_oracle as BO  # noqa: E402
from oracle import correspondence_oracle as CO  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NEW = ("pdsc_corr_batch_workspace_bytes", "pdsc_build_correspondences_batch", "pdsc_build_correspondences_batch_ex")


def g(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
    from pointdsc_amd import _lib
    import pointdsc_amd
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pointdsc_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for name in NEW:
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", header)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert getattr(lib, name) is not None and re.search(rf"\bT {name}\b", out), name
    assert callable(pointdsc_amd.build_correspondences_batch) and "build_correspondences_batch" in pointdsc_amd.__all__


def test_argument_checks():
    from pointdsc_amd import _lib
    from pointdsc_amd.correspondences import build_correspondences_batch
    desc = [torch.randn(5, 8), torch.randn(7, 8)]
    kp = [torch.randn(5, 3), torch.randn(7, 3)]
    with pytest.raises(RuntimeError, match="must live on the GPU"):                   # the package's usual error: no CPU path
        build_correspondences_batch(desc, kp, [(0, 1)])
    for bad in ([(0, 2)], [(-1, 0)], [(0, 1), (2, 1)], torch.tensor([[0, 5]])):
        with pytest.raises(ValueError, match="outside the pool"):
            build_correspondences_batch(desc, kp, bad)
    with pytest.raises(ValueError, match="non-empty"):
        build_correspondences_batch(desc, kp, [])
    with pytest.raises(ValueError, match="go together"):
        build_correspondences_batch(desc, kp, [(0, 1)], gt_trans=torch.eye(4)[None])
    with pytest.raises(ValueError, match="go together"):
        build_correspondences_batch(desc, kp, [(0, 1)], inlier_threshold=0.1)
    with pytest.raises(ValueError, match="descriptor length 65"):
        build_correspondences_batch([torch.randn(5, 65), torch.randn(7, 65)], kp, [(0, 1)])
    with pytest.raises(ValueError, match="metric"):
        build_correspondences_batch(desc, kp, [(0, 1)], metric="cosine")
    with pytest.raises(ValueError, match="cloud 1"):
        build_correspondences_batch(desc, [kp[0], torch.randn(6, 3)], [(0, 1)])
    # the C entry: bad arguments are refused with their text before anything is enqueued (no device is touched)
    lib = _lib.load()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(P=1, D=8, mutual=0, metric=0, tiles=1, max_tgt=7, cap=5, gt=None, labels=None, ws_bytes=1 << 20, splits=0, desc_ptr=p):
        return lib.pdsc_build_correspondences_batch_ex(desc_ptr, p, p, P, D, mutual, metric, tiles, max_tgt, cap, gt, 0.1, p, p, p, p, p,
                                                       labels, p, ws_bytes, splits, None)
    assert lib.pdsc_corr_batch_workspace_bytes(1, 1, 5) == 128 * 8 + 6 * 8
    assert lib.pdsc_corr_batch_workspace_bytes(3, 7, 2049) == 7 * 128 * 8 + 3 * 3 * 6 * 8
    assert lib.pdsc_corr_batch_workspace_bytes(0, 1, 5) == 0
    for kw, text in ((dict(D=65), "D=65"), (dict(P=0), "P=0"), (dict(desc_ptr=None), "null pointer"), (dict(mutual=1, tiles=1), "total_tiles=1"),
                     (dict(gt=p), "go together"), (dict(labels=p), "go together"), (dict(splits=2), "splits=2"), (dict(cap=0), "cap=0"),
                     (dict(metric=2), "metric=2")):
        assert call(**kw) == -1, kw                                                     # PDSC_ERR_ARG
        assert text in _lib.last_error() and _lib.last_error().startswith("pdsc_build_correspondences_batch:"), (kw, _lib.last_error())
    assert call(ws_bytes=128 * 8) == -2 and "workspace" in _lib.last_error()          # PDSC_ERR_WORKSPACE


def test_batch_oracle_on_a_hand_worked_case():
    """Four source points, three targets, orthogonal unit descriptors: s2t = [1, 0, 2, 1]; target 1's nearest source is 0 (the first of
    sources 0 and 3), so the mutual check drops source 3.  Pose: a shift of 0.2 along z."""
    e = np.eye(4, dtype=np.float32)
    desc = [np.stack([e[0], e[1], e[2], e[0]]), np.stack([e[1], e[0], e[2]])]
    kp = [np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32),
          np.array([[1, 0, 0.05], [0, 0, 0.2], [0, 1.5, 0]], np.float32)]
    T = np.eye(4)
    T[2, 3] = 0.2
    plain, mutual = (BO.build_correspondences_batch(desc, kp, [(0, 1), (0, 1)], use_mutual=m, gt_trans=np.stack([T, np.eye(4)]),
                                                    inlier_threshold=0.1) for m in (False, True))
    assert plain[0]["corr"].tolist() == [[0, 1], [1, 0], [2, 2], [3, 1]]
    assert mutual[0]["corr"].tolist() == [[0, 1], [1, 0], [2, 2]]
    # distances after the shift: |0.2 - 0.2| = 0, |0.2 - 0.05| = 0.15, sqrt(0.5^2 + 0.2^2), |1.2 - 0.2| = 1
    assert np.allclose(plain[0]["gt_dist"], [0.0, 0.15, np.sqrt(0.29), 1.0], atol=1e-7) and plain[0]["gt_dist"].dtype == np.float64
    assert plain[0]["gt_labels"].tolist() == [1, 0, 0, 0] and mutual[0]["gt_labels"].tolist() == [1, 0, 0]
    # identity pose (second entry): 0.2, 0.05, 0.5, 0.8
    assert plain[1]["gt_labels"].tolist() == [0, 1, 0, 0]
    mean = np.array([0.25, 0.25, 0.25, 0.25, 0.375, 0.1125], np.float32)
    want = np.concatenate([kp[0], kp[1][[1, 0, 2, 1]]], axis=1) - mean
    assert np.abs(plain[0]["corr_pos"] - want).max() < 1e-6


def test_label_threshold_is_the_double_rule():
    """np.float32(0.1) = 0.100000001490116 is GREATER than the double 0.10: a target at that distance is an outlier of
    datasets/ThreeDMatch.py:293-297 (fp64), the float32 just below it an inlier."""
    desc, kp, T, thr, want = BO.threshold_case()
    assert float(np.float32(0.1)) > 0.10 > float(np.nextafter(np.float32(0.1), np.float32(0)))
    res = BO.build_correspondences_batch(desc, kp, [(0, 1)], gt_trans=T, inlier_threshold=thr)[0]
    assert res["corr"].tolist() == [[0, 0], [1, 1]] and np.array_equal(res["gt_labels"], want)
    assert res["gt_dist"][0] == float(np.float32(0.1))                                # the identity pose changes nothing in fp64


def test_fp32_label_rule_differs_on_a_constructed_case():
    """harness.gt_labels_from_trans evaluates the same formula in fp32 torch (distance and threshold rounded to fp32): among seeded
    targets within 2e-8 of the threshold some are labelled differently from the fp64 rule.  This documents the difference between the
    two label paths; it is not a defect of the fp32 function."""
    from pointdsc_amd import harness
    rs = np.random.RandomState(0)
    ang = rs.uniform(0, 2 * np.pi, 4000)
    r = 0.1 + rs.uniform(-2e-8, 2e-8, 4000)
    tgt = np.stack([r * np.cos(ang), r * np.sin(ang), np.zeros(4000)], axis=1).astype(np.float32)
    src = np.zeros_like(tgt)
    _, l64 = BO.label_lines(src, tgt, np.eye(4), 0.10)
    l32 = harness.gt_labels_from_trans(torch.from_numpy(src), torch.from_numpy(tgt), torch.eye(4), 0.10).numpy()
    assert 0 < (l64 != l32).sum() < 4000 and 0 < l64.sum() < 4000


def test_label_seed_keeps_its_margin():
    """The seeded label case of the GPU test: no distance within 1e-9 of the threshold (so the fp64 device arithmetic, whose products
    are not fused where numpy's BLAS may fuse them, decides every label like the oracle), both labels present."""
    desc, kp = BO.make_pool(33)
    for mutual in (False, True):
        res = BO.build_correspondences_batch(desc, kp, BO.LABEL_PAIRS, use_mutual=mutual, gt_trans=BO.label_poses(),
                                             inlier_threshold=BO.LABEL_THR)
        dist = np.concatenate([r["gt_dist"] for r in res])
        lab = np.concatenate([r["gt_labels"] for r in res])
        assert np.abs(dist - BO.LABEL_THR).min() > 1e-9, np.abs(dist - BO.LABEL_THR).min()
        assert 0.05 < lab.mean() < 0.95 and len(lab) > 100, (lab.mean(), len(lab))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(d):
    desc, kp = BO.make_pool(d)
    return [g(a) for a in desc], [g(a) for a in kp]


@functools.lru_cache(maxsize=None)
def per_pair(d, mutual, metric):
    """The reference of the bitwise tests: build_correspondences per pair of POOL_PAIRS, computed once."""
    from pointdsc_amd.correspondences import build_correspondences
    desc, kp = pool(d)
    return [build_correspondences(desc[s], desc[t], kp[s], kp[t], use_mutual=mutual, metric=metric) for s, t in BO.POOL_PAIRS]


def batch_call(d, mutual, metric, splits=0, **kw):
    from pointdsc_amd.correspondences import build_correspondences_batch
    desc, kp = pool(d)
    return build_correspondences_batch(desc, kp, BO.POOL_PAIRS, use_mutual=mutual, metric=metric, _splits=splits, **kw)


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("d", [33, 32])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("mutual", [False, True])
def test_batch_equals_the_per_pair_entry_points_bit_for_bit(mutual, metric, d):
    """D = 33 takes the scalar staging path, D = 32 the 16-byte one.  Both routes take the correctly rounded fp64 mean, so corr_pos is
    bitwise equal as well; rows behind a pair's count are exactly zero in every output."""
    want = per_pair(d, mutual, metric)
    got = batch_call(d, mutual, metric)
    P, cap = len(BO.POOL_PAIRS), 700
    assert got["corr_pos"].shape == (P, cap, 6) and got["src_keypts"].shape == got["tgt_keypts"].shape == (P, cap, 3)
    assert got["corr"].shape == (P, cap, 2) and got["corr"].dtype == torch.int32
    assert got["num_corr"].shape == (P,) and got["num_corr"].dtype == torch.int32 and got["num_corr"].is_cuda
    counts = got["num_corr"].tolist()
    sizes = [int(pool(d)[0][s].shape[0]) for s, _ in BO.POOL_PAIRS]
    if mutual:
        assert got["num_corr_host"] is None and any(0 < c < n for c, n in zip(counts, sizes)), counts
    else:
        assert got["num_corr_host"] == counts == sizes
    for p, w in enumerate(want):
        n = counts[p]
        assert n == w["corr"].shape[0], (p, n)
        assert torch.equal(got["corr"][p, :n], w["corr"]), p
        assert torch.equal(got["src_keypts"][p, :n], w["src_keypts"][0]) and torch.equal(got["tgt_keypts"][p, :n], w["tgt_keypts"][0]), p
        assert torch.equal(got["corr_pos"][p, :n], w["corr_pos"][0]), (p, float((got["corr_pos"][p, :n] - w["corr_pos"][0]).abs().max()))
        for k in ("corr", "src_keypts", "tgt_keypts", "corr_pos"):
            assert not got[k][p, n:].any(), (p, k)
    # the two orders of a pair and the repeated pair: entries 3 and 4 are the same pair
    for k in ("corr", "corr_pos"):
        assert torch.equal(got[k][3], got[k][4])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [33, 32])
def test_target_split_does_not_change_a_bit(d):
    """_ex split override: 1 split, 2 (384 targets per split: the 700-row cloud's second range and the 257-row cloud's only range end
    inside a staged 128-row tile, the 1- and 77-row clouds leave the second split empty) and the maximum (6: one tile each)."""
    for metric in ("l2", "ip"):
        base = batch_call(d, True, metric, splits=1)
        for s in (2, 6, 0):
            assert_same_bits(batch_call(d, True, metric, splits=s), base)
        want = per_pair(d, True, metric)
        n = base["num_corr"].tolist()
        assert all(torch.equal(base["corr"][p, :n[p]], w["corr"]) for p, w in enumerate(want))
    with pytest.raises(RuntimeError, match="splits=7"):
        batch_call(d, True, "l2", splits=7)


@pytest.mark.gpu
def test_ties_inside_a_batch_resolve_like_numpy():
    """Equal distances -> the first index (np.argmin), for a cloud with exact duplicates placed between ordinary clouds; sizes that are
    no multiple of any tile and descriptor lengths 1, 8, 32, 64."""
    from pointdsc_amd.correspondences import build_correspondences_batch
    src, tgt, skp, tkp = CO.make_descriptors(131, 77, 33, seed=9)
    tgt[40] = tgt[3]                          # exact duplicates: both at the same distance from everybody
    tgt[76] = tgt[3]
    src[5] = tgt[3]
    o0, o1, k0, k1 = CO.make_descriptors(257, 200, 33, seed=21)
    desc, kp = [o0, src, tgt, o1], [k0, skp, tkp, k1]
    pairs = [(0, 3), (1, 2), (3, 0), (2, 1), (1, 3)]
    got = build_correspondences_batch([g(a) for a in desc], [g(a) for a in kp], pairs)
    for p, (s, t) in enumerate(pairs):
        want = np.argmin(CO.nn_distance_matrix(desc[s], desc[t]), axis=1)
        assert np.array_equal(got["corr"][p, :len(want), 1].cpu().numpy(), want), p
    assert int(got["corr"][1, 5, 1]) == 3
    for ns, nt, d in ((1, 1, 8), (5, 700, 32), (700, 5, 64), (257, 129, 1)):
        s, t, ks, kt = CO.make_descriptors(ns, nt, d, seed=ns + nt)
        o, _, ko, _ = CO.make_descriptors(150, 1, d, seed=5)
        res = build_correspondences_batch([g(o), g(s), g(t)], [g(ko), g(ks), g(kt)], [(0, 2), (1, 2), (2, 1), (1, 0)])
        for p, (a, b) in enumerate([(o, t), (s, t), (t, s), (s, o)]):
            dm = CO.nn_distance_matrix(a, b)
            idx = res["corr"][p, :len(a), 1].cpu().numpy()
            # compare through the distances (d = 1: many exact ties are legitimate, the index must still be a minimum)
            assert np.array_equal(idx, np.argmin(dm, axis=1)) or np.abs(dm[np.arange(len(a)), idx] - dm.min(axis=1)).max() < 1e-6, (ns, nt, d, p)


@pytest.mark.gpu
def test_near_ties_and_nan_inside_a_batch_resolve_like_numpy():
    """Candidates one ulp apart, two different radicands with the same rounded square root, chains of one-ulp improvements, inner
    products above 1 (NaN distances: the first of them wins) and a NaN descriptor, on inputs whose inner products are exact in any
    summation order -- as one cloud pair of a pool whose other pairs are ordinary.  The NaN cloud must not disturb its neighbours."""
    from pointdsc_amd.correspondences import build_correspondences_batch
    rs = np.random.RandomState(5)
    ns, nt, d = 200, 900, 16
    src = np.zeros((ns, d), np.float32)
    src[np.arange(ns), np.arange(ns) % 5] = 1.0                      # source i = unit vector of column i % 5
    tgt = np.zeros((nt, d), np.float32)
    tgt[:, :4] = rs.uniform(-0.6, 0.6, size=(nt, 4)).astype(np.float32)
    tgt[:, 4] = rs.uniform(-0.6, 0.2, size=nt).astype(np.float32)
    one = np.float32(0.75)

    def ulps(x, k, towards=2.0):
        x = np.float32(x)
        for _ in range(k):
            x = np.nextafter(x, np.float32(towards))
        return x
    tgt[100, 0], tgt[500, 0] = one, ulps(one, 1)                     # a later target one ulp closer than an earlier one
    tgt[50, 1], tgt[60, 1], tgt[700, 1] = ulps(one, 2), one, ulps(one, 1)      # the closer one first, near misses behind it
    for k in range(6):
        tgt[120 * k + 7, 2] = ulps(one, k)                           # a chain of improvements one ulp apart
    tgt[300, 3], tgt[200, 3], tgt[850, 3] = 1.5, 1.25, 3.0           # negative radicands: NaN distances, the first index wins
    tgt[80, 4], tgt[640, 4] = ulps(0.25, 4, towards=-2.0), np.float32(0.25)    # different radicands, the same rounded distance
    o0, o1, k0, k1 = CO.make_descriptors(300, 150, d, seed=31)
    kp_s, kp_t = rs.rand(ns, 3).astype(np.float32), rs.rand(nt, 3).astype(np.float32)
    pairs = [(0, 3), (1, 2), (3, 0)]                                 # the special pair between two ordinary ones
    results = []
    for case_nan in (False, True):
        t = tgt.copy()
        if case_nan:
            t[150, 0] = np.nan                                       # row 150: NaN distance for EVERY source (0 * NaN)
        desc = [o0, src, t, o1]
        got = build_correspondences_batch([g(a) for a in desc], [g(a) for a in (k0, kp_s, kp_t, k1)], pairs)
        results.append(got)
        for p, (a, b) in enumerate(pairs):
            with np.errstate(invalid="ignore"):
                want = np.argmin(CO.nn_distance_matrix(desc[a], desc[b]), axis=1)
            idx = got["corr"][p, :len(want), 1].cpu().numpy()
            assert np.array_equal(idx, want), (case_nan, p, np.flatnonzero(idx != want)[:8])
            if p == 1 and case_nan:
                assert (want == 150).all()
            elif p == 1:
                assert want[3] == 200 and want[4] == 80 and want[0] == 500 and want[1] == 50 and want[2] == 607, want[:5]
    for p in (0, 2):                                                 # the ordinary pairs: the same bits beside a NaN cloud
        for k in ("corr", "corr_pos", "src_keypts", "tgt_keypts"):
            assert torch.equal(results[0][k][p], results[1][k][p]), (p, k)


@pytest.mark.gpu
def test_labels_equal_the_fp64_oracle():
    from pointdsc_amd.correspondences import build_correspondences_batch
    desc_np, kp_np = BO.make_pool(33)
    desc, kp = pool(33)
    poses = BO.label_poses()
    for mutual in (False, True):
        want = BO.build_correspondences_batch(desc_np, kp_np, BO.LABEL_PAIRS, use_mutual=mutual, gt_trans=poses, inlier_threshold=BO.LABEL_THR)
        for gt in (torch.from_numpy(poses), g(poses)):                                     # fp64 on the host or on the device
            got = build_correspondences_batch(desc, kp, BO.LABEL_PAIRS, use_mutual=mutual, gt_trans=gt, inlier_threshold=BO.LABEL_THR)
            assert got["gt_labels"].shape == got["corr"].shape[:2] and got["gt_labels"].dtype == torch.float32
            n = got["num_corr"].tolist()
            for p, w in enumerate(want):
                assert n[p] == len(w["gt_labels"]) and np.array_equal(got["corr"][p, :n[p]].cpu().numpy(), w["corr"]), p
                assert np.array_equal(got["gt_labels"][p, :n[p]].cpu().numpy(), w["gt_labels"]), p
                assert not got["gt_labels"][p, n[p]:].any()
    # the threshold itself: float32(0.1) is outside the double 0.10, the float32 below it inside
    d2, k2, T, thr, lab = BO.threshold_case()
    got = build_correspondences_batch([g(a) for a in d2], [g(a) for a in k2], [(0, 1)], gt_trans=T, inlier_threshold=thr)
    assert got["corr"][0].tolist() == [[0, 0], [1, 1]] and np.array_equal(got["gt_labels"][0].cpu().numpy(), lab)
    got32 = build_correspondences_batch([g(a) for a in d2], [g(a) for a in k2], [(0, 1)], gt_trans=torch.eye(4)[None], inlier_threshold=thr)
    assert np.array_equal(got32["gt_labels"][0].cpu().numpy(), lab)                        # any float dtype is taken to fp64


@pytest.mark.gpu
def test_repeatable_and_without_a_host_read():
    """Two calls on the same inputs give equal bits, and the call completes under torch's sync debug mode "error" (every implicit
    device synchronisation raises): the wrapper builds its table from shapes and uploads it without waiting.  Where the installed
    torch has no such mode the property rests on review: the wrapper holds no .item() / .tolist() / .cpu() on a device tensor."""
    desc, kp = pool(33)
    poses = g(BO.label_poses())
    torch.cuda.synchronize()
    first = batch_call(33, True, "l2", gt_trans=poses[:1].expand(len(BO.POOL_PAIRS), 4, 4), inlier_threshold=BO.LABEL_THR)
    try:
        torch.cuda.set_sync_debug_mode("error")
        guarded = True
    except (AttributeError, RuntimeError):
        guarded = False
    try:
        second = batch_call(33, True, "l2", gt_trans=poses[:1].expand(len(BO.POOL_PAIRS), 4, 4), inlier_threshold=BO.LABEL_THR)
        plain = batch_call(33, False, "ip")
    finally:
        if guarded:
            torch.cuda.set_sync_debug_mode("default")
    assert_same_bits(first, second)
    assert plain["num_corr_host"] == [int(desc[s].shape[0]) for s, _ in BO.POOL_PAIRS]
    print(f"[corr_batch] sync debug mode available: {guarded}")


@functools.lru_cache(maxsize=None)
def demo_model():
    from pointdsc_amd import PointDSC, workloads
    model = PointDSC(**workloads.BASE_MODEL)
    model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    return model.eval().cuda()


@pytest.mark.gpu
def test_multiway_edges_in_groups_of_pairs():
    """Four views of the demo cloud: three loop-closure candidates go through one batched correspondence call, one ragged forward and
    one loop_closure_edge.  Same edges and flags as one pair per call; poses within the margin the project uses between a ragged and
    a one-pair-per-call forward (test_eval_loop_batches_pairs_of_different_size): RE 0.05 deg, TE 0.1 cm; info[5,5] within 2."""
    from oracle import pointdsc_oracle as O
    from pointdsc_amd import harness
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    views = harness.demo_views(cloud, 4)
    for mutual in (False, True):
        one = harness.multiway_edges(demo_model(), views, use_mutual=mutual, batch_pairs=1)
        many = harness.multiway_edges(demo_model(), views, use_mutual=mutual, batch_pairs=4)
        assert [(s, t, u) for s, t, _, _, u in one] == [(s, t, u) for s, t, _, _, u in many]
        assert any(u for _, _, _, _, u in one), "no loop closure survived the overlap gate"
        for (s, t, T1, i1, u), (_, _, T2, i2, _) in zip(one, many):
            re, te = O.registration_errors(torch.from_numpy(T2).float(), torch.from_numpy(T1).float())
            print(f"[corr_batch] mutual {mutual} edge {s} -> {t}: RE {float(re):.5f} deg TE {float(te):.5f} cm info55 {i1[5, 5]:.0f} / {i2[5, 5]:.0f}")
            assert float(re) < 0.05 and float(te) < 0.1, (s, t, float(re), float(te))
            assert abs(i1[5, 5] - i2[5, 5]) <= 2, (s, t)
            if not u:
                assert np.array_equal(T1, T2) and np.array_equal(i1, i2)                 # odometry edges do not pass through the batch


@pytest.mark.gpu
def test_eval_scene_with_batched_correspondences():
    """eval_scene(batch_size=4, corr_batch=True) against corr_batch=False: the bounds of test_eval_loop_batches_pairs_of_different_size."""
    from pointdsc_amd import harness
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    one = harness.eval_scene(demo_model(), harness.demo_pairs(cloud, 5, corrupt=0.3), use_mutual=True, batch_size=4)
    many = harness.eval_scene(demo_model(), harness.demo_pairs(cloud, 5, corrupt=0.3), use_mutual=True, batch_size=4, corr_batch=True)
    assert one.shape == many.shape == (5, 12)
    assert len(set(one[:, 3].astype(int).tolist())) > 1, "the pairs were meant to differ"
    assert (one[:, 0] == many[:, 0]).all() and (one[:, 0] == 1).all()
    print("[corr_batch] eval_scene RE/TE diff", np.abs(one[:, 1] - many[:, 1]).max(), np.abs(one[:, 2] - many[:, 2]).max())
    assert np.abs(one[:, 1] - many[:, 1]).max() < 0.05 and np.abs(one[:, 2] - many[:, 2]).max() < 0.1  # RE [deg], TE [cm]
    assert np.abs(one[:, [3, 5]] - many[:, [3, 5]]).max() <= 2                                           # inlier counts (in / true positives)
    assert np.abs(one[:, [4, 6, 7, 8]] - many[:, [4, 6, 7, 8]]).max() < 0.01                             # ratios / P / R / F1
    assert (many[:, 10] > 0).all() and len(set(many[:4, 10].tolist())) == 1                             # data time: the group's, per pair
