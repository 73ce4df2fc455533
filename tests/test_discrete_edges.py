"""f-23: the four discrete decisions of the forward's tail at their edges, against integer truth.

Every pose the forward returns passes through NMS (nms_flags_kernel, or nms_grid_kernel + nms_window_kernel), seed ranking
(seed_select_kernel), the seed kNN (knn_select_kernel or knn_fused_kernel) and the vote (score_kernel, select_best_kernel; the
inlier count of refine_kernel steers the refinement loop).  These kernels claim exactness -- "sqrt(x) < thr and x < x* are the same
predicate bit for bit", "the keys are bit-identical to nms_flags_kernel's", "the same selection on the same distance bits" -- and the
other tests hold them to it on random inputs only, with near-ties excused.  Here every input is DYADIC (tests/discrete_oracle.py):
the fp32 chains are exact, truth is integer arithmetic, and keys, seeds, neighbour lists, counts, the winner, its pose bits and its
labels are compared with assert_array_equal.  Nothing is excused and there is no tolerance anywhere in this file.

Sections: A threshold edges (36 thresholds over nine binades; residuals at x* - ulp, x*, x* + ulp through nms_keys, nms_keys_grid,
score_hypotheses and post_refinement), B NMS grid geometry, C seed ranking, D seed kNN in both forms, E voting sizes and ties, F the
CPU side (exactness rule, branch reach from the sources' constants, seeded defects).

Out of scope: NaN keys in rank_select (the kernel's order of NaN keys is whatever their bit patterns give; the forward's confidences
are finite or the range sentinel has fired).  One list cut cannot be placed where the issue lists it: a round adds at most 128
entries, so no list passes KF_CAP - 128 in round 0; "first" below is round 1, the earliest round a cut can happen.

Only pointdsc_amd.ops is called.  Every device test prints one line: case, branch reached, mismatches.
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
import discrete_oracle as D  # noqa: E402

F32 = np.float32
TCS = D.threshold_cases()
THR_IDS = [f"{float(t['thr']):.9g}" for t in TCS]
GEOMETRY = D.nms_geometry_cases()
NONFINITE = D.nms_nonfinite_cases()
RANK = D.rank_cases()
KNN = D.knn_cases()


def _id(name):
    return name.replace(" ", "_").replace(",", "").replace(":", "")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# references, computed once and shared
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nms_truth(kind, i):
    case = {"A": lambda: D.nms_threshold_cloud(TCS[i]), "B": lambda: GEOMETRY[i], "batch": lambda: D.nms_batch_case()[i]}[kind]()
    keys, exact = D.nms_truth_units(case["units"], case["conf"], case["n_star"])
    return case, keys, exact


@functools.lru_cache(maxsize=None)
def _vote_truth_a(i, winner):
    c = D.vote_threshold_case(TCS[i], winner)
    return c, D.vote_truth(c["R"], c["t"], c["P"], c["Q"], c["n_star"], c["m"], c["thr"])


@functools.lru_cache(maxsize=None)
def _vote_truth_e(S, N, seed, mode):
    c = D.vote_size_case(S, N, seed, mode)
    return c, D.vote_truth(c["R"], c["t"], c["P"], c["Q"], c["n_star"], c["m"], c["thr"])


E_CASES = [(S, N, 50 + i, "mixed") for i, (S, N) in enumerate(D.VOTE_SIZES)] + \
          [(1100, 257, 70, "tie"), (2049, 255, 73, "tie"), (1025, 64, 71, "zero"), (5, 1000, 72, "all")]


@functools.lru_cache(maxsize=None)
def _knn_truth(i):
    return D.knn_case_truth(KNN[i])


# ---------------------------------------------------------------------------------------------------------------------------
# F. CPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracles_by_hand():
    assert D.is_f32(1 << 40) and D.is_f32((1 << 24) - 1) and not D.is_f32((1 << 24) + 1) and D.is_f32((1 << 25) + 4)
    assert list(D.is_f32_array([0, 3 << 30, (1 << 24) + 1])) == [True, True, False]
    # x*(0.1f): sqrt is monotone, 0.01f's neighbour below has a root below 0.1f
    xs = D.x_star(0.1)
    assert np.sqrt(xs) >= F32(0.1) > np.sqrt(np.nextafter(xs, F32(0)))
    # four points on a line: 0 and 1 are 3 apart (inside R = 4), 2 is exactly R from 1, 3 is far; confidences 1 < 2, 3, 0
    P = np.array([[0, 0, 0], [3, 0, 0], [7, 0, 0], [100, 0, 0]], np.int64)
    keys, _ = D.nms_truth_units(P, np.array([1, 2, 3, -1], F32), 16)
    assert list(bits(keys)) == list(bits(np.array([0.0, 2, 3, -1], F32)))          # 0 suppressed by 1; 1 is exactly R from 2: kept
    keys, _ = D.nms_truth_units(P, np.array([-1, 2, 3, -1], F32), 16)
    assert bits(keys)[0] == bits(np.array([-0.0], F32))[0]                         # the sign of a suppressed negative is kept
    assert list(D.rank_truth(np.array([0.5, -0.0, 0.0, 2.0, 0.5], F32), 5)) == [3, 0, 4, 1, 2]
    assert list(D.knn_truth(np.array([[5, 1, 1, 0, 7]]), 3)[0]) == [1, 2, 0]       # rank 0 (index 3) dropped, ties by index


def test_threshold_list_realises_all_three_radicands_exactly():
    assert len(TCS) >= 32 and all(tc is not None for tc in TCS)
    thrs = [tc["thr"] for tc in TCS]
    assert len(set(map(float, thrs))) == len(thrs) and all(F32(t) in thrs for t in (0.1, 0.6, 1.2))
    assert len({math.frexp(float(t))[1] for t in thrs}) >= 8
    assert [float(F32(t)) for t in D.search_thresholds(len(TCS))] == [float(t) for t in thrs]      # the list is what the search finds
    # the issue's own figures
    t01 = D.threshold_case(0.1)
    assert t01["m"] == 15 and t01["n"] == (10737417, 10737418, 10737419) == (D.B_NSTAR - 1, D.B_NSTAR, D.B_NSTAR + 1)
    for trip, n in zip((D.B_IN, D.B_AT, D.B_OUT), t01["n"]):
        d2, exact = D.chain_exact(np.array(trip))
        assert int(d2) == n and bool(exact)
    assert D.threshold_case(0.6)["n"] == D.threshold_case(1.2)["n"] == (24159190, 24159192, 24159194)
    for tc in TCS:
        thr, m = tc["thr"], tc["m"]
        xs = tc["x_star"]
        ladder = [np.nextafter(xs, F32(0)), xs, np.nextafter(xs, F32(np.inf))]
        assert [bool(np.sqrt(v) < thr) for v in ladder] == [True, False, False]
        for kind in range(3):
            for v in D.offset_variants(tc["offsets"][kind], 12):
                d2, exact = D.chain_exact(v)
                assert bool(exact) and int(d2) == tc["n"][kind]
                # ... and the same chain in float32: products and sums formed in fp64 (exact there) and rounded once per fma
                f = (v.astype(np.float64) * 2.0 ** -m).astype(F32).astype(np.float64)
                r = F32(f[0] * f[0])
                r = F32(f[1] * f[1] + float(r))
                r = F32(f[2] * f[2] + float(r))
                assert r == ladder[kind]
    print(f"[f23] {len(TCS)} thresholds, binades {sorted({math.frexp(float(t))[1] for t in thrs})}, quanta 2^-{min(t['m'] for t in TCS)} .. "
          f"2^-{max(t['m'] for t in TCS)}")


def test_exactness_rule_holds_for_every_case():
    """Every intermediate of every crafted case is an fp32 value or, for the squared distances that decide nothing, far from x*
    (discrete_oracle.radicand_check); the deciding pairs are exact.  The oracles assert while they compute."""
    exact_pairs = 0
    for i in range(len(TCS)):
        case, keys, exact = _nms_truth("A", i)
        assert np.array_equal(bits(keys) != bits(case["conf"]), case["expect_suppressed"]) and exact >= 24 + 2 * len(case["P"])
        exact_pairs += exact
        for w in range(3):
            c, (counts, best, labels, ex) = _vote_truth_a(i, w)
            assert best == w and int(labels.sum()) == counts[best] == 7 and ex >= len(c["P"])
        for kind in range(3):
            c = D.refine_threshold_case(TCS[i], kind)
            counts, _, labels, ex = D.vote_truth(c["R"], c["t"], c["P"], c["Q"], c["n_star"], c["m"], c["thr"])
            assert ex == 64 and counts[0] == labels.sum() == (64 if kind == 0 else 0)
    for i in range(len(GEOMETRY)):
        exact_pairs += _nms_truth("B", i)[2]
    for i in range(3):
        exact_pairs += _nms_truth("batch", i)[2]
    for c in NONFINITE:                                  # the lattice part of these clouds (all rows but one)
        rows = np.arange(len(c["P"])) != c["bad_row"]
        units = np.round(c["P"][rows].astype(np.float64) * 2.0 ** D.B_M).astype(np.int64)
        assert np.array_equal(D.to_f32(units, D.B_M), c["P"][rows])
        D.nms_truth_units(units, c["conf"][rows], c["n_star"])
    for e in E_CASES:
        _vote_truth_e(*e)
    for i, case in enumerate(KNN):
        dist, _ = _knn_truth(i)
        assert all(np.abs(d).max() < 1 << 21 for d in dist)                        # 2 - 2 dot within 21 bits of 2^-12
    for case in RANK:
        assert np.isfinite(case["keys"]).all() or "inf" in case["name"]
        assert not np.isnan(case["keys"]).any()
    print(f"[f23] exactness: {exact_pairs} exact NMS pairs, the rest far from x*; kNN rows on 2^-6, distances on 2^-12")


def test_every_case_reaches_its_branch():
    c = D.source_constants()
    assert (c["NMS2_ROWS"], c["NMS2_MAX_SLICE"], c["GRID_MAX"], c["SEL_THREADS"], c["SC_SEEDS"]) == (512, 2048, 64, 1024, 4)
    assert (c["KNN_FAST_CAP"], c["KF_CAP"], c["KF_KEEP"], c["KF_MAX_WANT"], c["KF_ROWS"]) == (1024, 256, 96, 48, 32)
    lines = []
    # B: the grid header and the cell table of every geometry case
    for case in GEOMETRY:
        keys, info = D.nms_model(case)
        want = case["branch"]
        for k in ("nbx", "nby", "floor_x", "floor_y", "wx"):
            if k in want:
                assert float(info[k]) == float(want[k]), (case["name"], k, info[k])
        if "min_per_cell" in want:
            assert info["max_per_cell"] >= want["min_per_cell"] > c["SEL_THREADS"]
        if "suppressed" in want:
            assert int((bits(keys) != bits(case["conf"])).sum()) == want["suppressed"]
        if want.get("negative"):
            assert (case["units"] < 0).any()
        if "size" in want:
            n = want["size"]
            rows, splits, sl = D.n2_launch(n)
            assert rows == -(-n // c["NMS2_ROWS"]) and sl <= c["NMS2_MAX_SLICE"] and splits * sl >= n
        cx, cy = D.grid_cells_exact(case["units"], case["m"], info)
        assert np.array_equal(cx, info["cx"]) and np.array_equal(cy, info["cy"])      # the float32 index == the rational floor
        lines.append(f"{case['name']}: {len(case['P'])} points, floor {info['floor_x']:.0f} x {info['floor_y']:.0f} -> cells "
                     f"{info['nbx']} x {info['nby']}, most in a cell {info['max_per_cell']}")
    b1 = D.nms_model(GEOMETRY[0])[1]
    u = GEOMETRY[0]["units"]
    on_face = (u[:, 0] % 4096 == 0) & (u[:, 0] > 0) & (u[:, 0] < 8 * D.U)
    below = u[:, 0] % 4096 == 4095
    assert on_face.sum() >= 8 and below.sum() >= 8 and (b1["cx"][on_face] == u[on_face, 0] // 4096).all()
    assert (b1["cx"][below] == u[below, 0] // 4096).all()
    # pairs inside the radius in neighbouring cells in x, in y and diagonally; two cells apart just above R
    d2, _ = D.chain_exact(u[:, None, :] - u[None, :, :])
    inside = d2 < D.B_NSTAR
    ddx, ddy = b1["cx"][None, :] - b1["cx"][:, None], b1["cy"][None, :] - b1["cy"][:, None]
    assert (inside & (ddx == 1) & (ddy == 0)).any() and (inside & (ddx == 0) & (ddy == 1)).any() and (inside & (ddx == 1) & (ddy == 1)).any()
    b2, u2 = D.nms_model(GEOMETRY[1])[1], GEOMETRY[1]["units"]
    d2, _ = D.chain_exact(u2[:, None, :] - u2[None, :, :])
    two_apart = (np.abs(b2["cx"][None, :] - b2["cx"][:, None]) == 2) | (np.abs(b2["cy"][None, :] - b2["cy"][:, None]) == 2)
    assert (two_apart & (d2 == 3330 ** 2)).sum() >= 12 and 3330 ** 2 > D.B_NSTAR
    for case in NONFINITE:
        info = D.nms_model(case)[1]
        assert info["bad"] and info["nbx"] == info["nby"] == 1
    assert [D.nms_model(cs)[1]["nbx"] for cs in D.nms_batch_case()] == [10, 64, 1]
    # A: the threshold clouds use the grid proper
    for i in range(len(TCS)):
        info = D.nms_model(_nms_truth("A", i)[0])[1]
        assert info["nbx"] >= 9 and info["nby"] >= 6
    # C: where the S-th value's run of equal keys lies
    for case in RANK:
        _, info = D.rank_model(case["keys"], case["S"])
        for k, v in case["branch"].items():
            if k in info:
                assert info[k] == v, (case["name"], k, info)
        if case["branch"].get("crosses"):
            assert info["last_chunk"] > info["first_chunk"] and info["run"] > 700 and 0 < info["taken"] < info["run"]
        if case["branch"].get("low_byte"):
            assert len({int(b) >> 8 for b in bits(case["keys"])}) == 1
        if case["branch"].get("top_byte"):
            assert len({int(b) & 0xFFFFFF for b in bits(np.abs(case["keys"]))}) <= 6
        if case["branch"].get("lds_limit"):
            assert case["S"] * 8 == 128 * 1024
        lines.append(f"{case['name']}: N {len(case['keys'])} S {case['S']}, run of {info['run']} equal keys in chunks "
                     f"{info['first_chunk']}..{info['last_chunk']}, {info['taken']} taken, the last in chunk {info['last_taken_chunk']}")
    # D: paths of the matrix form, rounds and cuts of the fused form
    seen = {"first": False, "middle": False, "last": False, "exact": False, "late": False, "overflow": False, "block_map": False}
    for i, case in enumerate(KNN):
        dist, truth = _knn_truth(i)
        n, k, want = case["codes"].shape[1], case["k"], case["branch"]
        paths, cuts, exact_cuts, late, surv = set(), set(), set(), 0, 0
        for b in range(len(dist)):
            for s in range(min(len(dist[b]), 6)):
                if "matrix" in case["forms"]:
                    got, info = D.knn_matrix_model(dist[b][s], k)
                    assert np.array_equal(got, truth[b][s])
                    paths.add(info["path"])
                    surv = max(surv, info["survivors"] or 0)
                if "fused" in case["forms"]:
                    assert k + 1 <= c["KF_MAX_WANT"] and n >= 256
                    got, info = D.knn_fused_model(dist[b][s], k)
                    assert np.array_equal(got, truth[b][s])
                    last = info["rounds"] - 1
                    cuts |= {"first" if r == 1 else "last" if r == last and info["partial_last_round"] else "middle" for r in info["bound_cuts"]}
                    exact_cuts |= set(info["exact_cuts"])
                    late += info["late_ties"]
        if "path" in want:
            assert paths == {want["path"]}, (case["name"], paths)
        if "min_survivors" in want:
            assert surv >= want["min_survivors"] > c["KNN_FAST_CAP"]
            seen["overflow"] = True
        if "cut_rounds" in want:
            assert set(want["cut_rounds"]) <= cuts, (case["name"], cuts)
        if want.get("exact_cut"):
            assert exact_cuts
        if want.get("late_ties"):
            assert late > 100
        if want.get("self_not_rank0"):
            assert sum(int(np.argsort(dist[0][s], kind="stable")[0] != case["seeds"][0][s]) for s in range(len(case["seeds"][0]))) >= 4
        if want.get("negative"):
            assert min(d.min() for d in dist) < 0 and any((d == 0).any() for d in dist)
        if want.get("block_map"):
            assert len(dist) % 8 == 0 and not np.array_equal(case["codes"][0], case["codes"][1])
            seen["block_map"] = True
        for r in cuts:
            seen[r] = True
        seen["exact"] |= bool(exact_cuts)
        seen["late"] |= late > 0
        lines.append(f"{case['name']}: matrix {sorted(paths)} (most survivors {surv}), fused cuts {sorted(cuts)} exact-ranking cut "
                     f"{bool(exact_cuts)} late ties {late}")
    assert all(seen.values()), seen
    # the boundary min(64, ceil(N / 4)) >= k + 1 at k = 40: 160 columns are 40 groups (radix), 161 are 41 (fast)
    assert [next(cs["branch"]["path"] for cs in KNN if cs["name"].startswith(f"D3 fast-path boundary N={n} ")) for n in (160, 161, 164, 165)] == \
        ["radix", "fast", "fast", "fast"]
    # E: padded groups and ties
    for e in E_CASES:
        _, (counts, best, labels, _) = _vote_truth_e(*e)
        S, N, _, mode = e
        if mode == "tie":
            assert counts[5] == counts[5 + 1024] == counts.max() and best == 5
        if mode == "zero":
            assert counts.max() == 0 and best == 0
        if mode == "all":
            assert counts.max() == N
        lines.append(f"E S={S} N={N} {mode}: best {best} with {counts[best]} votes ({int((counts == counts[best]).sum())} equal), "
                     f"padded slots {(-S) % c['SC_SEEDS']}")
    assert {(-S) % c["SC_SEEDS"] for S, *_ in E_CASES} == {0, 1, 3}
    for line in lines:
        print("[f23]", line)


def test_every_seeded_defect_is_rejected_by_a_case():
    rejected = {}
    nms_cases = [(c, _nms_truth("B", i)[1]) for i, c in enumerate(GEOMETRY) if len(c["P"]) <= 600] + \
                [_nms_truth("A", i)[:2] for i in (0, 1, 2, 7, 20)]
    for defect in D.NMS_DEFECTS:
        rejected[defect] = [c["name"] for c, truth in nms_cases if D.same_key_bits(D.nms_model(c, (defect,))[0], truth)]
    # the cell index is invisible in the keys (any monotone index with unit steps gives a superset window): the defect is held by
    # the cell table, against the rational floor
    assert rejected["trunc_index"] == []
    for c in GEOMETRY:
        h = D.grid_header(c["P"], c["R"])
        cx, cy = D.grid_cells(c["P"], h, ("trunc_index",))
        ex, ey = D.grid_cells_exact(c["units"], c["m"], h)
        if not (np.array_equal(cx, ex) and np.array_equal(cy, ey)):
            rejected["trunc_index"].append(c["name"] + " (cell table)")
    for defect in D.RANK_DEFECTS:
        rejected[defect] = [c["name"] for c in RANK[:-1]
                            if not np.array_equal(D.rank_model(c["keys"], c["S"], (defect,))[0], D.rank_truth(c["keys"], c["S"]))]
    for defect in D.KNN_DEFECTS:
        rejected[defect] = []
        for i, case in enumerate(KNN):
            dist, truth = _knn_truth(i)
            for form, model in (("matrix", D.knn_matrix_model), ("fused", D.knn_fused_model)):
                if form in case["forms"] and any(
                        not np.array_equal(model(dist[0][s], case["k"], case["seeds"][0][s], (defect,))[0], truth[0][s])
                        for s in range(min(len(dist[0]), 6))):
                    rejected[defect].append(f"{case['name']} ({form})")
    for defect in D.VOTE_DEFECTS:
        rejected[defect] = []
        for e in E_CASES:
            _, (counts, best, _, _) = _vote_truth_e(*e)
            got_counts, got_best = D.vote_model(counts, (defect,))
            if got_best != best or not np.array_equal(got_counts, counts):
                rejected[defect].append(f"E S={e[0]} N={e[1]} {e[3]}")
    assert len(rejected) == 15
    for defect, by in rejected.items():
        print(f"[f23] defect {defect}: rejected by {len(by)} cases, e.g. {by[:3]}")
        assert by, defect
    # the threshold defects are rejected by EVERY threshold cloud, the tie defects by the cases built for them
    assert all(f"A thr={float(TCS[i]['thr']):.9g}" in rejected[d] for i in (0, 1, 2) for d in ("le_threshold", "radicand_low",
                                                                                                "radicand_high", "fp64_square"))
    assert any("D2" in n for n in rejected["fast_cap_lost"]) and any("D7" in n for n in rejected["cut_ignores_index"])
    assert any("tie" in n for n in rejected["argmax_last"]) and any("-0.0" in n for n in rejected["negative_zero_below"])


# ---------------------------------------------------------------------------------------------------------------------------
# device tests
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype).contiguous()


def _ops():
    from pointdsc_amd import ops
    return ops


def _nms_both(P, conf, R):
    ops = _ops()
    P, conf = _dev(P), _dev(conf)
    n2 = ops.nms_keys(P, conf, float(R)).cpu().numpy()
    grid = ops.nms_keys_grid(P, conf, float(R)).cpu().numpy()
    return n2, grid


def _report(name, branch, mismatches):
    print(f"[f23] {name}: {branch}, mismatches = {mismatches}")
    assert mismatches == 0, name


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TCS)), ids=THR_IDS)
def test_nms_at_the_threshold(i):
    """A: i is suppressed iff its distance to the stronger j is x* - ulp; at x* and at x* + ulp it stays; keys as int32 bits."""
    case, truth, _ = _nms_truth("A", i)
    n2, grid = _nms_both(case["P"][None], case["conf"][None], case["R"])
    bad = D.same_key_bits(n2, truth) + D.same_key_bits(grid, truth)
    sup = bits(n2[0]) != bits(case["conf"])
    assert np.array_equal(sup, case["expect_suppressed"])
    assert np.array_equal(bits(n2[0])[sup], bits(case["conf"][sup] * F32(0)))      # conf * 0 with the sign kept
    info = D.nms_model(case)[1]
    _report(case["name"] + " nms", f"x* = {TCS[i]['n'][1]} * 4^-{TCS[i]['m']}, cells {info['nbx']} x {info['nby']}, 4 suppressed of 12 pairs", bad)


def _check_vote(name, branch, cases_truths, thr):
    """One score_hypotheses call over a batch of cases of one shape; counts, best, pose bits and labels against the truth."""
    ops = _ops()
    T = np.stack([D.transforms_f32(c["R"], c["t"], c["m"]) for c, _ in cases_truths])
    P = np.stack([D.to_f32(c["P"], c["m"]) for c, _ in cases_truths])
    Q = np.stack([D.to_f32(c["Q"], c["m"]) for c, _ in cases_truths])
    counts, best, initial, labels = (x.cpu().numpy() for x in ops.score_hypotheses(_dev(T), _dev(P), _dev(Q), float(thr)))
    bad = 0
    for b, (c, (tcounts, tbest, tlabels, _)) in enumerate(cases_truths):
        bad += int((counts[b] != tcounts).sum()) + int(best[b] != tbest) + int((bits(initial[b]) != bits(T[b, tbest])).sum())
        bad += int((bits(labels[b]) != bits(tlabels)).sum()) + int(labels[b].sum() != counts[b, best[b]])
    _report(name, branch, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TCS)), ids=THR_IDS)
def test_score_and_labels_at_the_threshold(i):
    """A: the radicand form (score_kernel) and the norm3 form (select_best_kernel) on the same rows: counts equal the integer truth and
    labels.sum() == counts[best], with each of the three edge hypotheses made the winner in turn."""
    for w in range(3):
        c, truth = _vote_truth_a(i, w)
        _check_vote(f"A thr={THR_IDS[i]} score, winner {w}", f"counts {list(map(int, truth[0]))}, 3 rows at x* and 3 above it per hypothesis",
                    [(c, truth)], c["thr"])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TCS)), ids=THR_IDS)
def test_refinement_at_the_threshold(i):
    """A: all rows at x*: no inlier, the loop stops before its first solve and returns the input pose bits; all rows at x* - ulp:
    at least one solve; max_iters = 0: the input bits."""
    ops = _ops()
    out = []
    for kind in range(3):
        c = D.refine_threshold_case(TCS[i], kind)
        T0 = D.transforms_f32(c["R"], c["t"], c["m"])
        args = (_dev(T0), _dev(D.to_f32(c["P"], c["m"])[None]), _dev(D.to_f32(c["Q"], c["m"])[None]), float(c["thr"]))
        final, solves = ops.post_refinement(*args, max_iters=20)
        final0, solves0 = ops.post_refinement(*args, max_iters=0)
        out.append((int(solves[0]), int((bits(final.cpu().numpy()) != bits(T0)).sum())))
        assert int(solves0[0]) == 0 and np.array_equal(bits(final0.cpu().numpy()), bits(T0))
    bad = int(out[0][0] < 1) + int(out[1] != (0, 0)) + int(out[2] != (0, 0))
    _report(f"A thr={THR_IDS[i]} refine", f"solves {out[0][0]} / {out[1][0]} / {out[2][0]} with all rows below / at / above x*", bad)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(GEOMETRY)), ids=[_id(c["name"]) for c in GEOMETRY])
def test_nms_grid_geometry(i):
    """B: nms_keys_grid == nms_keys == integer truth as int32 bits."""
    case, truth, _ = _nms_truth("B", i)
    n2, grid = _nms_both(case["P"][None], case["conf"][None], case["R"])
    info = D.nms_model(case)[1]
    _report(case["name"], f"cells {info['nbx']} x {info['nby']}, most in a cell {info['max_per_cell']}, "
            f"{int((bits(truth) != bits(case['conf'])).sum())} of {len(truth)} suppressed",
            D.same_key_bits(n2, truth) + D.same_key_bits(grid, truth) + D.same_key_bits(grid, n2))


@pytest.mark.gpu
def test_nms_batch_of_three_clouds():
    cases = D.nms_batch_case()
    truth = np.stack([_nms_truth("batch", b)[1] for b in range(3)])
    n2, grid = _nms_both(np.stack([c["P"] for c in cases]), np.stack([c["conf"] for c in cases]), D.B_R)
    _report("B9 bs=3", "cells 10 x 10, 64 x 64 and 1 x 1 in one call", D.same_key_bits(n2, truth) + D.same_key_bits(grid, truth))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(NONFINITE)), ids=[_id(c["name"]) for c in NONFINITE])
def test_nms_with_a_non_finite_coordinate(i):
    """B: the grid falls back to one cell and equals the N^2 kernel and the truth; a NaN distance is not >= R, so it suppresses i
    exactly when conf_i >= conf_j fails."""
    case = NONFINITE[i]
    truth = D.nms_truth_float(case["P"], case["conf"], D.x_star(case["R"]))
    n2, grid = _nms_both(case["P"][None], case["conf"][None], case["R"])
    _report(case["name"], f"one cell, {int((bits(truth) != bits(case['conf'])).sum())} of {len(truth)} suppressed",
            D.same_key_bits(n2, truth) + D.same_key_bits(grid, truth))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(RANK)), ids=[_id(c["name"]) for c in RANK])
def test_rank_select(i):
    """C: seeds == sorted(range(N), key=(-key with -0.0 == +0.0, index))[:S]."""
    case = RANK[i]
    got = _ops().rank_select(_dev(case["keys"][None]), case["S"]).cpu().numpy()[0]
    info = D.rank_model(case["keys"], case["S"])[1]
    _report(case["name"], f"run of {info['run']} equal keys over chunks {info['first_chunk']}..{info['last_chunk']}, {info['taken']} taken",
            int((got != D.rank_truth(case["keys"], case["S"])).sum()))


@pytest.mark.gpu
def test_rank_select_batch_and_limit():
    ops = _ops()
    cases = [RANK[3], RANK[8], RANK[2]]                   # three different key sets, cut to one length
    n = min(len(c["keys"]) for c in cases)
    keys = np.stack([c["keys"][:n] for c in cases])
    got = ops.rank_select(_dev(keys), 700).cpu().numpy()
    _report("C9 bs=3", f"N {n} S 700", sum(int((got[b] != D.rank_truth(keys[b], 700)).sum()) for b in range(3)))
    with pytest.raises(RuntimeError, match=r"num_seeds=16385 exceeds the single-workgroup LDS list \(16384\)"):
        ops.rank_select(_dev(np.zeros((1, 16385), F32)), 16385)
    torch.cuda.synchronize()


def _knn_forms(case, x, truth, name):
    ops = _ops()
    normed, seeds = _dev(x), _dev(case["seeds"], torch.int32)
    bad, ran = 0, []
    for form in case["forms"]:
        got = ops.knn_seeds(normed, seeds, case["k"], form=form).cpu().numpy()
        bad += int((got != truth).sum())
        ran.append(form)
    if case["pf"] and "fused" in case["forms"]:
        got = ops.knn_seeds(normed, seeds, case["k"], form="fused", normed_pf=_dev(D.pf_image(x))).cpu().numpy()
        bad += int((got != truth).sum())
        ran.append("fused+pf")
    return bad, ran


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(KNN)), ids=[_id(c["name"]) for c in KNN])
def test_knn_seeds(i):
    """D: every neighbour list == stable sort of (integer distance, index), ranks 1 .. k, in every form the case lists."""
    case = KNN[i]
    _, truth = _knn_truth(i)
    bad, ran = _knn_forms(case, D.knn_features(case), truth, case["name"])
    _report(case["name"], f"forms {'/'.join(ran)}, {truth.shape[0]} x {truth.shape[1]} seeds", bad)


@pytest.mark.gpu
def test_knn_seeds_with_nan_rows():
    """D: rows with a NaN of either sign; every seed keeps k + 1 finite distances; NaN ranks last, as torch.sort has it."""
    case, x, truth, nan_rows = D.knn_nan_case()
    bad, ran = _knn_forms(case, x, truth[None], case["name"])
    _report(case["name"], f"forms {'/'.join(ran)}, {len(nan_rows)} NaN rows", bad)


@pytest.mark.gpu
@pytest.mark.parametrize("e", E_CASES, ids=[f"S{e[0]}_N{e[1]}_{e[3]}" for e in E_CASES])
def test_vote_sizes_and_ties(e):
    """E: counts, best (lowest index among equal counts), initial_trans bits and labels."""
    c, truth = _vote_truth_e(*e)
    counts, best = truth[0], truth[1]
    _check_vote(f"E S={e[0]} N={e[1]} {e[3]}", f"best {best} with {counts[best]} votes, {int((counts == counts[best]).sum())} equal", [(c, truth)],
                c["thr"])


@pytest.mark.gpu
def test_vote_batch_of_three():
    group = [_vote_truth_e(1100, 257, seed, mode) for seed, mode in ((56, "mixed"), (80, "tie"), (81, "zero"))]
    _check_vote("E bs=3 S=1100 N=257", "mixed / tie / all-zero pairs in one call", group, D.B_R)
