"""f-20: the radius search of csrc/icp_grid.h and the voxel keys of csrc/voxel.hip at their edges, against exact brute force.

icp_grid.h claims that its hashed 27-cell search "equals brute force exactly".  The ICP, multiway and FPFH tests run it on
room-scale clouds only; here the device runs the branches those never reach -- the cell cap, queries one cell outside the box,
heavy hash collisions, degenerate boxes, the strict fp32 radius rule at equality, exact ties between distinct points, the
streaming selection of nb_search_kernel, voxel faces and the 2^20 voxel limit -- on inputs whose arithmetic is exact (see
tests/grid_oracle.py), so that indices, counts, d2 and sums are compared bit for bit and no point is excused.

Three entry points observe the search: information_matrix(return_correspondences=True) and registration_icp(max_iteration=0)
(nearest target within a radius, section A), hybrid_neighbours (lists, section B); voxel_down_sample and
voxel_down_sample_with_normals observe the keys (section C).  A call takes ONE radius, so "all cases as one ragged batch" is one
batch of all pairs per distinct radius, each pair compared with its solo call at its own radius.

Bounds.  Dyadic cases: bit equality (the CPU test asserts that every sum stays within 53 bits of its quantum, so every order of
summation is exact); inlier_rmse within 1 ulp of sqrt(exact sum / n) (division and square root are correctly rounded, bit
equality is expected and the distance is printed).  Seeded fp32 cases: the oracle's margins >= NEAR_TIE are asserted first;
the information matrix within the reorder bound n 2^-52 sum|terms| of tests/test_multiway.py; sum d2 is a sum of n positive
terms, so any order is within n 2^-53 relative of the exact one and the rmse within (n 2^-53 + 2^-52) relative of the oracle's
(half the sum's error through the square root, plus the roundings of the division and the root on both sides).
"""
from __future__ import annotations

import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT / "tests") not in sys.path:
    sys.path.insert(0, str(ROOT / "tests"))
import grid_oracle as G  # noqa: E402
from test_icp import NEAR_TIE  # noqa: E402
from test_multiway import information_oracle  # noqa: E402

CASES = G.nearest_cases()
CASE_IDS = [c["name"].split()[0] for c in CASES]
POSES = ("identity", "translation")
LIST_CASES = G.list_cases()
LIST_PARAMS = [(i, k) for i, c in enumerate(LIST_CASES) if not c["name"].startswith("B5") for k in c["max_nn"]]
VOXEL_CASES = G.voxel_cases()


# ---------------------------------------------------------------------------------------------------------------------------
# references, computed once and shared
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(ci, vi):
    """The oracle of case ci under pose vi: corr, count, information (exact or with its reorder bound), sum d2, rmse, margin."""
    case = CASES[ci]
    _, S, T = G.pose_variants(case)[vi]
    P, Q = G.apply_pose(T, G.f64(S)), G.f64(case["Q"])
    corr, d2 = G.nearest_oracle(P, Q, case["r"])
    n = int((corr >= 0).sum())
    ref = {"S": S, "T": T, "P": P, "corr": corr, "n": n, "margin": None, "bound": None}
    if case["quantum"]:
        ref["info"], ref["info_bits"] = G.info_exact(Q, corr, case["quantum"])
        ref["sum_d2"], ref["d2_bits"] = G.sum_d2_exact(P, Q, corr, case["quantum"])
    else:
        o = information_oracle(S, case["Q"], T, case["r"])
        ref["info"], ref["bound"], ref["margin"] = o["info"], n * 2.0 ** -52 * o["abs_terms"], o["margin"]
        ref["oracle_corr"] = o["corr"]
        ref["sum_d2"] = math.fsum(d2[corr >= 0])
    ref["rmse"] = G.rmse_of(ref["sum_d2"], n)
    return ref


@functools.lru_cache(maxsize=None)
def _list_reference(i, max_nn):
    c = LIST_CASES[i]
    return G.lists_oracle(G.f64(c["P"]), c["r"], max_nn)


@functools.lru_cache(maxsize=None)
def _models():
    consts = G.source_constants()
    return consts, [G.GridModel(c["Q"], c["r"], consts) for c in CASES], [G.GridModel(c["P"], c["r"], consts) for c in LIST_CASES]


# ---------------------------------------------------------------------------------------------------------------------------
# D. CPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_self_checks_by_hand():
    Q = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]], np.float64)
    P = np.array([[0.25, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [3, 0, 0], [1.5, 0, 0], [1.0, 0.25, 0]])
    corr, d2 = G.nearest_oracle(P, Q, 0.5)
    # 0.25 from target 0; 0.5 from targets 0, 1, 3: exactly r, strict '<' excludes all; sqrt(0.5) away; far; exactly r from 1 and 3;
    # 0.25 from the duplicated targets 1 and 3: the lowest index
    assert list(corr) == [0, -1, -1, -1, -1, 1]
    assert list(d2) == [0.0625, 0, 0, 0, 0, 0.0625]
    corr, d2 = G.nearest_oracle(P, Q, 0.75)
    assert list(corr) == [0, 0, 0, -1, 1, 1] and d2[1] == 0.25 and d2[2] == 0.5      # ties 0 / 1 / 3 and 0 / 1 / 2: index 0
    # lists: ascending (d2, index), self included, cut at max_nn, strict radius
    L = np.array([[0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [1, 0, 0], [0, 0, 0]], np.float64)
    idx, d2, count = G.lists_oracle(L, 1.0, 4)
    assert list(idx[0]) == [0, 5, 1, 2] and list(d2[0]) == [0, 0, 0.25, 0.25] and count[0] == 4      # the cut falls inside the tie shell 1, 2, 3
    assert list(idx[5]) == [0, 5, 1, 2]                                                              # a copy's list starts with the lower index
    assert list(idx[4]) == [4, 1, -1, -1] and count[4] == 2 and list(d2[4]) == [0, 0.25, 0, 0]         # 0 and 5 are exactly r away
    idx, _, count = G.lists_oracle(L, 1.0, 1)
    assert list(idx[:, 0]) == [0, 1, 2, 3, 4, 0] and (count == 1).all()
    # the radius is float32(r r): for r = 0.05 * 1.4 it is larger than r r in fp64, and a distance between the two is inside
    r = 0.05 * 1.4
    a = float(np.float32(0.07))
    assert r * r < a * a < G.radius2(r) < float(np.nextafter(np.float32(0.07), np.float32(1))) ** 2
    # integer sums
    info, bits = G.info_exact(np.array([[1, 2, 3], [-1, 0, 2], [0.5, -0.5, 0]]), np.array([0, 1, 2]), G.Q10)
    assert info[0, 0] == 17.25 and info[0, 1] == -1.75 and info[1, 3] == 5.0 and info[5, 5] == 3.0 and bits <= 53
    np.testing.assert_array_equal(info, info.T)
    total, _ = G.sum_d2_exact(np.array([[0.25, 0, 0], [9, 9, 9.0]]), Q, np.array([0, -1]), G.Q10)
    assert total == 0.0625


def test_voxel_oracle_by_hand_and_against_the_harness():
    from pointdsc_amd import harness
    # voxel 1/8 anchored at min - 1/16: points 0 and 1/16 apart on a face fall into voxels 0 and 1; -1/16 .. 0 share a voxel
    P = np.array([[0, 0, 0], [0.0625, 0, 0], [0.125, 0, 0], [0.1875, 0, 0]], np.float32) - np.float32(1.0)
    N = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0.5, 0]], np.float64)
    pts, nrm, keys = G.voxel_oracle(P, N, 0.125)
    assert list(keys) == [0, 1, 2]
    np.testing.assert_array_equal(pts[:, 0], np.array([-1.0, -0.90625, -0.8125], np.float32))
    np.testing.assert_array_equal(nrm[1], [0, 0.5, 0.5])
    consts = G.source_constants()
    for c in VOXEL_CASES:
        idx = G.voxel_model(c["P"], c["voxel"], consts["voxel_max"])
        assert (idx is not None) == c["accepted"], c["name"]
        if c["accepted"]:
            pts, _, keys = G.voxel_oracle(c["P"], c["normals"], c["voxel"], idx)
            np.testing.assert_array_equal(pts, harness.voxel_down_sample(c["P"], c["voxel"]), err_msg=c["name"])
            assert np.all(np.diff(keys) > 0)


def test_dyadic_cases_are_on_their_quantum_and_inside_their_bit_budget():
    for ci, case in enumerate(CASES):
        if not case["quantum"]:
            continue
        for vi, (tag, S, T) in enumerate(G.pose_variants(case)):
            ref = _reference(ci, vi)
            for a in (case["Q"], S, ref["P"]):
                G.to_ints(a, case["quantum"])                                   # asserts the quantum
                assert np.abs(a).max() <= 2.0 ** 9
            # the translation is exact: the device sees the same transformed source under both poses
            np.testing.assert_array_equal(ref["P"], G.f64(case["S"]), err_msg=case["name"])
            np.testing.assert_array_equal(ref["corr"], _reference(ci, 0)["corr"])
            print(f"[f20] {case['name']} {tag}: information {ref['info_bits']} bits, sum d2 {ref['d2_bits']} bits")
            assert ref["info_bits"] <= 53 and ref["d2_bits"] <= 53, (case["name"], ref["info_bits"], ref["d2_bits"])
    for c in LIST_CASES:
        if c["quantum"]:
            G.to_ints(c["P"], c["quantum"])
            assert np.abs(c["P"]).max() <= 2.0 ** 9
    for c in VOXEL_CASES:
        G.to_ints(c["P"], G.Q10 / 2)
        G.to_ints(c["normals"], G.Q10 / 2)
        assert np.abs(c["P"]).max() <= 2.0 ** 9 and len(c["P"]) * 2 ** 20 < 2 ** 53       # sums of <= 2^20 quanta each


def test_cases_reach_the_branches_they_are_listed_for():
    consts, models, list_models = _models()
    by = dict(zip(CASE_IDS, range(len(CASES))))
    count = lambda k: _reference(by[k], 0)["n"]                                        # noqa: E731
    reach = lambda k: models[by[k]].reach(_reference(by[k], 0)["P"])                   # noqa: E731
    for ci, case in enumerate(CASES):
        m = models[ci]
        print(f"[f20] {case['name']}: {len(case['S'])} x {len(case['Q'])} points, cells {tuple(int(v) for v in m.n)} cap taken "
              f"{m.cap_taken} buckets {m.buckets}, correspondences {_reference(ci, 0)['n']}, queries in a -1 / n cell "
              f"{m.reach(_reference(ci, 0)['P'])['outside']}")
        assert len(case["S"]) <= 2100 and len(case["Q"]) <= 2100
    # A1 / A2: the counts of the issue; most of the overhang is in a -1 / n cell; A2 has eight-way ties
    assert count("A1") == 512 and count("A2") == 637 and len(CASES[by["A1"]]["S"]) == 1728
    assert reach("A1")["outside"] > 500 and reach("A2")["outside"] > 500
    d2 = G.sqdist(_reference(by["A2"], 0)["P"], G.f64(CASES[by["A2"]]["Q"]))
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) == 8).any()
    assert (np.abs(d2 - G.radius2(0.51)) > 1e-3 * G.radius2(0.51)).all()               # no lattice distance near float32(r r)
    # A1: sources exactly r from a face
    assert (np.abs(G.sqdist(_reference(by["A1"], 0)["P"], G.f64(CASES[by["A1"]]["Q"])).min(axis=1) - 0.25) == 0).any()
    # A3: isolated targets; per target six sources at exactly r (excluded) and six just inside; the included targets sit in the
    # query's own cell or one cell away -- and two cells away once a cell is narrower than r (the defect 'narrow_cell')
    shell = CASES[by["A3"]]
    Q, P = G.f64(shell["Q"]), _reference(by["A3"], 0)["P"]
    dq = np.sqrt(G.sqdist(Q, Q) + np.eye(len(Q)) * 1e9)
    assert dq.min() >= 4 * shell["r"]
    corr = _reference(by["A3"], 0)["corr"]
    assert (corr >= 0).sum() == 6 * len(Q) and (np.sort(G.sqdist(P, Q), axis=1)[corr < 0, 0] == 0.25).all()
    m = models[by["A3"]]
    qc = np.floor((P - m.lo) / m.w)
    owner = np.repeat(np.arange(len(Q)), 12)
    away = np.abs(qc - m.target_cell[owner]).max(axis=1)
    assert set(away[corr >= 0].tolist()) == {0.0, 1.0} and away[corr < 0].max() == 1
    narrow = G.GridModel(shell["Q"], shell["r"], consts, ("narrow_cell",))
    assert narrow.w < shell["r"] - G.Q10
    assert np.abs(np.floor((P - narrow.lo) / narrow.w) - narrow.target_cell[owner]).max(axis=1)[corr >= 0].max() == 2
    # A4: the cap is taken
    m = models[by["A4"]]
    assert m.cap_taken and m.n.max() > 2 ** 20 and m.w > CASES[by["A4"]]["r"] * (1 + consts["cell_margin"])
    assert count("A4") > 100
    # A5: 64 buckets for more than 10^9 cells; some query has two of its 27 cells in one bucket
    m = models[by["A5"]]
    assert m.buckets == 64 == consts["hash_min"] and float(np.prod(m.n.astype(np.float64))) > 1e9 and reach("A5")["shared_bucket"] > 0
    assert 100 < count("A5") < 160
    # A6: one cell; a line and a plane of cells; a single target / source
    assert tuple(models[by["A6a"]].n) == (1, 1, 1) and _reference(by["A6a"], 0)["corr"].max() == 0
    assert tuple(models[by["A6b"]].n[1:]) == (1, 1) and models[by["A6b"]].n[0] > 1 and models[by["A6c"]].n[2] == 1
    assert len(CASES[by["A6d"]]["Q"]) == 1 and len(CASES[by["A6e"]]["S"]) == 1 and count("A6e") == 1
    assert reach("A6b")["outside"] > 0 and reach("A6c")["outside"] > 0
    # A7: the first source is a correspondence only under the fp32-rounded squared radius
    assert list(_reference(by["A7"], 0)["corr"]) == [0, -1] == list(_reference(by["A7"], 1)["corr"])
    assert G.sqdist(_reference(by["A7"], 0)["P"], np.zeros((1, 3)))[0, 0] > CASES[by["A7"]]["r"] ** 2
    assert count("A8") > 150 and np.abs(CASES[by["A8"]]["Q"]).min() > 2000

    # B: candidates per query, selections per query, ties at the cuts, points at exactly r
    for li, c in enumerate(LIST_CASES):
        P = G.f64(c["P"])
        cand = (G.sqdist(P, P) < G.radius2(c["r"])).sum(axis=1)
        m = list_models[li]
        print(f"[f20] {c['name']}: {len(P)} points, cells {tuple(int(v) for v in m.n)} cap taken {m.cap_taken} buckets {m.buckets}, "
              f"candidates per query {cand.min()} .. {cand.max()}")
        assert len(P) <= 2100
    P = G.f64(LIST_CASES[0]["P"])
    d2 = G.sqdist(P, P)
    cand = (d2 < 1.0).sum(axis=1)
    assert cand.min() == 51 and cand.max() == 251 and cand.max() > consts["cap"] - consts["wave"]
    assert 1 <= (d2 == 1.0).sum(axis=1).max() <= 3 + 3                                 # up to three per direction sign at exactly r
    interior = int(np.argmax(cand))
    s = np.sort(d2[interior])
    for cut in (30, 64, 100, 128):
        assert s[cut - 1] == s[cut], cut                                                 # ranks cut - 1 / cut: equal d2
    _, _, count, nsel = list_models[0].lists(128)
    assert nsel.max() >= 2 and (count == np.minimum(cand, 128)).all()
    P = G.f64(LIST_CASES[1]["P"])
    idx, d2l, count = _list_reference(1, 128)
    assert (idx[:300] == np.arange(128)).all() and not d2l[:300].any() and (count == 128).all()
    P = G.f64(LIST_CASES[2]["P"])
    assert ((G.sqdist(P, P) < 1.0).sum(axis=1) == 700).all()                              # 700 candidates: several selections
    assert list_models[2].lists(100)[3][:8].min() >= 3
    assert list_models[3].cap_taken and list_models[4].reach(G.f64(LIST_CASES[4]["P"]))["shared_bucket"] > 0
    assert len(LIST_CASES[5]["P"]) > 2 * consts["chunk"] and len(LIST_CASES[5]["P"]) <= 2100

    # C: integers before the floor; the limit on both sides; a run across a chunk and a tile boundary
    c = VOXEL_CASES[0]
    P = G.f64(c["P"])
    x = (P - (P.min(axis=0) - 0.5 * c["voxel"])) / c["voxel"]
    assert (x == np.floor(x)).mean() > 0.3 and P.max() <= 0 and P.min() < 0
    idx = G.voxel_model(VOXEL_CASES[1]["P"], G.Q10, consts["voxel_max"])
    assert idx[:, 0].max() + 1 == consts["voxel_max"] == 2 ** 20 and int(np.argmax(idx[:, 0])) == len(idx) - 1
    assert G.voxel_model(VOXEL_CASES[2]["P"], G.Q10, consts["voxel_max"]) is None
    c = VOXEL_CASES[3]
    idx = G.voxel_model(c["P"], c["voxel"], consts["voxel_max"])
    dims = idx.max(axis=0) + 1
    keys = np.sort((idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2])
    values, first, counts = np.unique(keys, return_index=True, return_counts=True)
    k = int(np.argmax(counts))
    assert counts[k] >= 1500 and first[k] > 0 and first[k] + counts[k] < len(keys) and len(values) > 10
    assert first[k] < consts["tile"] < consts["chunk"] < first[k] + counts[k] and len(keys) > consts["chunk"]


def _nearest_rejects(defect, consts):
    for ci, case in enumerate(CASES):
        ref = _reference(ci, 0)
        corr, d2 = G.GridModel(case["Q"], case["r"], consts, (defect,)).nearest(ref["P"])
        if not (np.array_equal(corr, ref["corr"]) and np.array_equal(d2[corr >= 0], G.nearest_oracle(ref["P"], G.f64(case["Q"]), case["r"])[1][corr >= 0])):
            return case["name"]
    return None


def _lists_reject(defect, consts, order=(1, 4, 3, 0, 2)):
    for li in order:
        c = LIST_CASES[li]
        for max_nn in c["max_nn"]:
            idx, d2, count, _ = G.GridModel(c["P"], c["r"], consts, (defect,)).lists(max_nn)
            want = _list_reference(li, max_nn)
            if not (np.array_equal(idx, want[0]) and np.array_equal(d2, want[1]) and np.array_equal(count, want[2])):
                return f"{c['name']} max_nn {max_nn}"
    return None


def test_model_without_defects_equals_brute_force_on_every_case():
    consts, models, list_models = _models()
    for ci, case in enumerate(CASES):
        for vi in range(2):
            ref = _reference(ci, vi)
            corr, d2 = models[ci].nearest(ref["P"])
            np.testing.assert_array_equal(corr, ref["corr"], err_msg=case["name"])
            np.testing.assert_array_equal(d2, G.nearest_oracle(ref["P"], G.f64(case["Q"]), case["r"])[1])
    for li, c in enumerate(LIST_CASES):
        for max_nn in c["max_nn"]:
            idx, d2, count, _ = list_models[li].lists(max_nn)
            want = _list_reference(li, max_nn)
            np.testing.assert_array_equal(idx, want[0], err_msg=c["name"])
            np.testing.assert_array_equal(d2, want[1], err_msg=c["name"])
            np.testing.assert_array_equal(count, want[2], err_msg=c["name"])


@pytest.mark.parametrize("defect", G.DEFECTS)
def test_every_seeded_defect_is_rejected_by_a_case(defect):
    """A condition on the cases, not a goal: a defect that no case rejects means a case is missing."""
    consts = _models()[0]
    nearest_defects = {"radius_le", "radius_fp64", "tie_highest", "cells_26", "no_outside_cells", "narrow_cell"}
    if defect == "voxel_trunc":
        hits = []
        for c in VOXEL_CASES:
            if not c["accepted"]:
                continue
            good = G.voxel_oracle(c["P"], c["normals"], c["voxel"])
            bad_idx = G.voxel_model(c["P"], c["voxel"], consts["voxel_max"], (defect,))
            bad = G.voxel_oracle(c["P"], c["normals"], c["voxel"], bad_idx) if bad_idx is not None else None
            if bad is None or bad[0].shape != good[0].shape or not np.array_equal(bad[0], good[0]):
                hits.append(c["name"])
        by = hits[0] if hits else None
    elif defect in nearest_defects:
        by = _nearest_rejects(defect, consts)
    else:
        by = _lists_reject(defect, consts)
    print(f"[f20] defect {defect}: rejected by {by}")
    assert by is not None, defect
    if defect == "narrow_cell":
        assert by.startswith("A3")                               # the radius shell is the case that is there for it


def test_seeded_cases_keep_their_margins():
    for ci, case in enumerate(CASES):
        if case["quantum"]:
            continue
        for vi, tag in enumerate(POSES):
            ref = _reference(ci, vi)
            print(f"[f20] {case['name']} {tag}: margin {ref['margin']:.2e} correspondences {ref['n']}")
            assert ref["margin"] >= NEAR_TIE, (case["name"], tag, ref["margin"])
            np.testing.assert_array_equal(ref["oracle_corr"], ref["corr"])          # the margin oracle and brute force agree
            assert ref["n"] > 0
    for c in LIST_CASES:
        if not c["quantum"]:
            margin = G.lists_margin(G.f64(c["P"]), c["r"])
            print(f"[f20] {c['name']}: list margin {margin:.2e}")
            assert margin >= NEAR_TIE, (c["name"], margin)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _gpu_info(S_list, Q_list, T_list, r):
    from pointdsc_amd import information_matrix
    res = information_matrix([_dev(s) for s in S_list], [_dev(q) for q in Q_list], r, _dev(np.stack(T_list)), return_correspondences=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _gpu_icp(S_list, Q_list, T_list, r):
    from pointdsc_amd import registration_icp
    res = registration_icp([_dev(s) for s in S_list], [_dev(q) for q in Q_list], _dev(np.stack(T_list)), max_correspondence_distance=r,
                           max_iteration=0)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if torch.is_tensor(v)}


@functools.lru_cache(maxsize=None)
def _solo(entry, ci, vi):
    ref = _reference(ci, vi)
    run = _gpu_info if entry == "info" else _gpu_icp
    return run([ref["S"]], [CASES[ci]["Q"]], [ref["T"]], CASES[ci]["r"])


@pytest.mark.gpu
@pytest.mark.parametrize("pose", range(2), ids=POSES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_information_correspondences_equal_brute_force(ci, pose):
    case, ref = CASES[ci], _reference(ci, pose)
    if ref["margin"] is not None:
        assert ref["margin"] >= NEAR_TIE, ref["margin"]
    got = _solo("info", ci, pose)
    info, ns = got["information"][0], len(ref["S"])
    print(f"[f20] {case['name']} {POSES[pose]}: information_matrix correspondences {int(got['num_correspondences'][0])} / {ns} "
          f"(oracle {ref['n']}) max|d info| {np.abs(info - ref['info']).max():.3e}")
    np.testing.assert_array_equal(got["correspondences"][0][:ns], ref["corr"])
    assert int(got["num_correspondences"][0]) == ref["n"]
    assert info[3, 3] == info[4, 4] == info[5, 5] == float(ref["n"])
    if case["quantum"]:
        assert ref["info_bits"] <= 53
        np.testing.assert_array_equal(info, ref["info"])
    else:
        assert (np.abs(info - ref["info"]) <= ref["bound"]).all(), np.abs(info - ref["info"]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("pose", range(2), ids=POSES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_icp_evaluation_at_zero_iterations_equals_brute_force(ci, pose):
    case, ref = CASES[ci], _reference(ci, pose)
    if ref["margin"] is not None:
        assert ref["margin"] >= NEAR_TIE, ref["margin"]
    got = _solo("icp", ci, pose)
    n, ns = ref["n"], len(ref["S"])
    rmse = float(got["inlier_rmse"][0])
    ulp = G.ulp_distance_f64(rmse, ref["rmse"])
    print(f"[f20] {case['name']} {POSES[pose]}: registration_icp num_corr {int(got['num_correspondences'][0])} / {ns} (oracle {n}) "
          f"rmse {rmse:.17g} ulp distance {ulp}")
    assert int(got["num_correspondences"][0]) == n
    assert float(got["fitness"][0]) == (n / ns if n else 0.0)
    if case["quantum"]:
        assert ref["d2_bits"] <= 53 and ulp <= 1, (rmse, ref["rmse"], ulp)
    else:
        assert abs(rmse - ref["rmse"]) <= (n * 2.0 ** -53 + 2.0 ** -52) * ref["rmse"], (rmse, ref["rmse"])
    assert int(got["iterations"][0]) == 0
    np.testing.assert_array_equal(got["transformation"][0], ref["T"])
    np.testing.assert_array_equal(got["transformation_f64"][0], ref["T"].astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["info", "icp"])
def test_all_cases_as_one_ragged_batch_equal_their_solo_calls_bitwise(entry):
    pairs = [(ci, vi) for ci in range(len(CASES)) for vi in range(2)]
    S_list = [_reference(ci, vi)["S"] for ci, vi in pairs]
    Q_list = [CASES[ci]["Q"] for ci, _ in pairs]
    T_list = [_reference(ci, vi)["T"] for ci, vi in pairs]
    assert len({len(s) for s in S_list}) > 4 and len({len(q) for q in Q_list}) > 4
    run = _gpu_info if entry == "info" else _gpu_icp
    compared = 0
    for r in sorted({c["r"] for c in CASES}):
        batch = run(S_list, Q_list, T_list, r)
        for b, (ci, vi) in enumerate(pairs):
            if CASES[ci]["r"] != r:
                continue
            alone, ns = _solo(entry, ci, vi), len(S_list[b])
            for k, v in alone.items():
                if k == "correspondences":
                    np.testing.assert_array_equal(batch[k][b][:ns], v[0][:ns], err_msg=f"{CASES[ci]['name']} {k}")
                    assert (batch[k][b][ns:] == -1).all()
                else:
                    np.testing.assert_array_equal(batch[k][b], v[0], err_msg=f"{CASES[ci]['name']} {POSES[vi]} {k}")
            compared += 1
    assert compared == len(pairs)


def _gpu_lists(clouds, r, max_nn, path):
    from pointdsc_amd.features import hybrid_neighbours
    res = hybrid_neighbours([_dev(p) for p in clouds], r, max_nn, path=path)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_lists(name, got, b, want, n):
    idx, d2, count = want
    print(f"[f20] {name}: list counts {int(got['count'][b][:n].min())} .. {int(got['count'][b][:n].max())} (oracle {count.min()} .. {count.max()})")
    np.testing.assert_array_equal(got["count"][b][:n], count, err_msg=name)
    np.testing.assert_array_equal(got["idx"][b][:n], idx, err_msg=name)
    np.testing.assert_array_equal(got["d2"][b][:n], d2, err_msg=name)
    assert (got["count"][b][n:] == 0).all() and (got["idx"][b][n:] == -1).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("li,max_nn", LIST_PARAMS, ids=[f"{LIST_CASES[i]['name'].replace(' ', '_')}-{k}" for i, k in LIST_PARAMS])
def test_neighbour_lists_equal_brute_force(li, max_nn):
    c = LIST_CASES[li]
    if not c["quantum"]:
        assert G.lists_margin(G.f64(c["P"]), c["r"]) >= NEAR_TIE
    got = _gpu_lists([c["P"]], c["r"], max_nn, "one")
    _check_lists(f"{c['name']} max_nn {max_nn}", got, 0, _list_reference(li, max_nn), len(c["P"]))


@pytest.mark.gpu
def test_neighbour_lists_path_many_equal_path_one_and_brute_force():
    c = LIST_CASES[5]
    max_nn = c["max_nn"][0]
    short = LIST_CASES[1]["P"]
    want = {len(c["P"]): _list_reference(5, max_nn), len(short): G.lists_oracle(G.f64(short), c["r"], max_nn)}
    results = {}
    for path in ("one", "many"):
        alone = _gpu_lists([c["P"]], c["r"], max_nn, path)
        _check_lists(f"{c['name']} path {path}", alone, 0, want[len(c["P"])], len(c["P"]))
        # a ragged batch with a short second cloud: its padding rows are empty lists
        batch = _gpu_lists([c["P"], short], c["r"], max_nn, path)
        _check_lists(f"{c['name']} path {path}, in a batch", batch, 0, want[len(c["P"])], len(c["P"]))
        _check_lists(f"{c['name']} path {path}, the short cloud", batch, 1, want[len(short)], len(short))
        assert len(short) < len(c["P"])
        results[path] = (alone, batch)
    for k in ("idx", "d2", "count"):
        np.testing.assert_array_equal(results["one"][0][k], results["many"][0][k], err_msg=k)
        np.testing.assert_array_equal(results["one"][1][k], results["many"][1][k], err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("vi", range(len(VOXEL_CASES)), ids=[c["name"].replace(" ", "_") for c in VOXEL_CASES])
def test_voxel_keys_and_means_equal_the_integer_oracle(vi):
    from pointdsc_amd import harness, voxel_down_sample
    from pointdsc_amd.features import voxel_down_sample_with_normals
    c = VOXEL_CASES[vi]
    n = len(c["P"])
    out, counts = voxel_down_sample([_dev(c["P"])], c["voxel"])
    torch.cuda.synchronize()
    out, counts = out.cpu().numpy()[0], counts.cpu().numpy()
    with_normals = {}
    for path in ("one", "many"):
        p, nrm, cnt = voxel_down_sample_with_normals([_dev(c["P"])], _dev(c["normals"][None], np.float64), c["voxel"], path=path)
        torch.cuda.synchronize()
        with_normals[path] = (p.cpu().numpy()[0], nrm.cpu().numpy()[0], int(cnt.cpu().numpy()[0]))
    if not c["accepted"]:
        # beyond 2^20 voxels on an axis: the header's contract, count 0 and zero rows
        print(f"[f20] {c['name']}: refused, count {int(counts[0])}")
        assert counts[0] == 0 and not out.any()
        for path, (p, nrm, cnt) in with_normals.items():
            assert cnt == 0 and not p.any() and not nrm.any(), path
        return
    pts, nrm, keys = G.voxel_oracle(c["P"], c["normals"], c["voxel"])
    np.testing.assert_array_equal(pts, harness.voxel_down_sample(c["P"], c["voxel"]))
    m = len(pts)
    print(f"[f20] {c['name']}: {n} -> {int(counts[0])} points (oracle {m})")
    assert counts[0] == m and out.shape == (n, 3)
    np.testing.assert_array_equal(out[:m].view(np.int32), pts.view(np.int32))
    assert not out[m:].any()
    for path, (p, nr, cnt) in with_normals.items():
        assert cnt == m and p.shape[0] == m, path
        np.testing.assert_array_equal(p.view(np.int32), pts.view(np.int32), err_msg=path)
        np.testing.assert_array_equal(nr, nrm, err_msg=path)
    if c["name"].startswith("C2"):
        np.testing.assert_array_equal(out[m - 1], c["P"][-1])                    # the far point's voxel is the last one
