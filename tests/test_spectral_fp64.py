"""The evaluation side path -- the spectral-matching baseline (baselines.SM), baselines.cal_confidence and ops.eval_stats; csrc/spectral.hip
and csrc/metrics.hip -- against the fp64 oracles of tests/spectral_oracle.py, at the sizes where the kernels' tilings break.

Error measure of a quantity X: err(X) = max|X - X64| / max|X64|.  Yardstick: e32, the same measure for the same lines in fp32 torch on
the CPU.  Bound: err <= max(4 e32, floor) (spectral_oracle.bound; the floors are the tolerances of the fixture tests).  Every device
test prints e32, the bound and the device's error per case before it asserts.

The CPU part holds what the GPU part rests on: the oracles reproduce the recorded reference outputs, every seeded case meets its
input conditions (so that no GPU assertion is vacuous), each deliberate defect of the table in test_*_defects is rejected by the check,
and the library refuses bad arguments before any HIP call.
"""
import ctypes as C
import math
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectral_oracle as S  # noqa: E402
from oracle import pointdsc_oracle as O  # noqa: E402
from oracle import sm_oracle  # noqa: E402
from pointdsc_amd import synthetic  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"
DEV = "cuda:0"
F64 = torch.float64
SM_CASES = [(n, regime) for n in S.SM_SIZES for regime in S.SM_REGIMES]
SM_IDS = [f"N{n}_{regime}" for n, regime in SM_CASES]


def g(t):
    return t.to(DEV).contiguous()


def cap(n):
    """At most 1 % of N labels, rounded up, may be undecided (or flip)."""
    return math.ceil(0.01 * n)


@pytest.fixture(scope="module")
def built_lib():
    from pointdsc_amd import build
    build.build(verbose=False)
    from pointdsc_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the oracles against the recorded reference outputs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sm_n257", "sm_n2000", "sm_kitti_n1500"])
def test_sm_oracle64_reproduces_reference_fixture(name):
    fx = np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    n, thr, scale = int(fx["N"]), float(fx["thr"]), float(fx["scale"])
    pair = synthetic.make_pair(n, seed=int(fx["seed"]), inlier_ratio=float(fx["inlier_ratio"]), scale=scale, noise=float(fx["noise"]))
    v64 = S.sm_power64(S.sm_matrix64(pair["corr_pos"][0], thr), 10)
    _, _, v32 = sm_oracle.sm_baseline(pair["corr_pos"][0], pair["src_keypts"][0], pair["tgt_keypts"][0], thr)
    assert S.err(v32, v64) < 2e-6                                   # the tolerance of test_sm_baseline_matches_reference_golden
    num_top = int(n * 0.1)
    labels, ref_labels = S.sm_select(v64, num_top), torch.from_numpy(fx["ref_pred_labels"][0])
    cut = float(torch.sort(v64, descending=True).values[num_top - 1])
    decided = (v64 - cut).abs() > 4e-6 * float(v64.abs().max())
    assert torch.equal(labels[decided], ref_labels[decided])
    flips = int((labels != ref_labels).sum())
    assert flips <= 2 * int((~decided).sum())
    T64 = S.pose(pair["src_keypts"][0], pair["tgt_keypts"][0], v64 * labels.to(F64), F64)
    tol = 1e-4 if flips == 0 else 3e-3
    assert (T64 - torch.from_numpy(fx["ref_pred_trans"][0]).to(F64)).abs().max() < tol * max(1.0, scale / 3.0)


def test_sm_yardstick_is_the_committed_fp32_oracle():
    """sm_power on sm_oracle.sm_matrix is sm_oracle.sm_baseline's eigenvector bit for bit, and sm_select is torch.sort's order."""
    for n, regime, it in ((21, "indoor", 2), (257, "outdoor", 10), (1027, "indoor", 1)):
        c = S.sm_case(n, regime)
        _, labels, v32 = sm_oracle.sm_baseline(c["corr"], c["src"], c["tgt"], c["thr"], top_ratio=0.1, num_iterations=it)
        assert torch.equal(v32, c["v32"][it])
        assert torch.equal(labels, S.sm_select(v32, int(n * 0.1)))
    v = torch.tensor([0.5, float("nan"), 0.5, 2.0, float("nan"), -1.0, 0.5])
    assert S.sm_order(v).tolist() == torch.sort(v, descending=True, stable=True).indices.tolist() == [1, 4, 3, 0, 2, 6, 5]
    assert S.sm_select(torch.full((6,), float("nan")), 2).tolist() == [1, 1, 0, 0, 0, 0]


def test_cal_confidence_oracle64_reproduces_reference_fixture():
    fx = np.load(GOLDEN / "confidence.npz", allow_pickle=False)
    for ci in range(int(fx["num_cases"])):
        n, seed, scale, sigma = int(fx[f"c{ci}_n"]), int(fx[f"c{ci}_seed"]), float(fx[f"c{ci}_scale"]), float(fx[f"c{ci}_sigma"])
        pair = synthetic.make_pair(n, seed=seed, inlier_ratio=0.3, scale=scale, noise=scale / 300.0)
        M = O.spatial_compat(pair["src_keypts"][0], pair["tgt_keypts"][0], torch.tensor([sigma]))[1]
        v = torch.from_numpy(fx[f"c{ci}_leading_eig"])[0]
        for k, method in enumerate(S.CC_METHODS):
            got, want = S.cal_confidence64(M, v, method, 10), float(fx[f"c{ci}_conf"][k])
            assert abs(got - want) / abs(want) < (1e-4 if method == "eig_value_ratio" else 2e-6), (n, method, got, want)


def test_eval_row64_reproduces_reference_fixture():
    fx = np.load(GOLDEN / "metrics.npz", allow_pickle=False)
    stats = S.eval_row64(*(torch.from_numpy(fx[k]) for k in ("trans", "gt_trans", "pred_labels", "gt_labels")), 15.0, 30.0).numpy()
    ref = fx["ref_stats"]
    assert np.array_equal(stats[:, 0], ref[:, 0])
    assert np.array_equal(stats[:, 3], ref[:, 3]) and np.array_equal(stats[:, 5], ref[:, 5])
    assert np.abs(stats[:, 1] - ref[:, 1]).max() < 2e-2
    assert np.abs(stats[:, 2] - ref[:, 2]).max() < 1e-3
    assert np.abs(stats[:, [4, 6, 7, 8]] - ref[:, [4, 6, 7, 8]]).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: input conditions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,regime", SM_CASES, ids=SM_IDS)
def test_sm_input_conditions(n, regime):
    """Per case and iteration count: a non-zero eigenvector (but for the one all-zero matrix), a yardstick within 1e-3 of fp64, and at
    most 1 % of the labels undecided at every top_ratio.  Seeds are 900 + N; (5, outdoor) has no compatible pair at seed 905 -- it
    would be a second all-zero matrix -- and takes seed 2905."""
    c = S.sm_case(n, regime)
    assert c["seed"] == S.SM_SEEDS.get((n, regime), 900 + n)
    for it in S.sm_iters(n):
        v64, e32, b = c["v64"][it], c["e32"][it], c["bound"][it]
        mx = float(v64.abs().max())
        und = [int(S.undecided(v64, int(n * r), b * mx).sum()) for r in S.SM_TOP_RATIOS]
        print(f"SM N={n} {regime} iters={it}: max|v64| {mx:.3e}  e32 {e32:.2e}  bound {b:.2e}  undecided {und} (cap {cap(n)})")
        if (n, regime) == S.SM_ALL_ZERO:
            assert mx == 0.0 and float(c["M64"].abs().max()) == 0.0
        else:
            assert mx > 0.0
        assert e32 < S.E32_MAX and bool(torch.isfinite(v64).all())
        assert max(und) <= cap(n)
    assert [int(n * r) for r in S.SM_TOP_RATIOS][::2] == [0, n]            # num_top reaches 0 and N


def test_sm_tie_and_nonfinite_inputs_are_what_they_claim():
    for n in (40, 300):
        for equal in (False, True):
            corr = S.tie_case(n, equal)
            M = S.sm_matrix64(corr, 0.10)
            a, b_ = n // 2, (n // 2 if equal else (n // 2 + 1) // 2)
            sums = M.sum(dim=1)
            assert torch.equal(sums[1::2], torch.full((a,), 4.5 * (a - 1), dtype=F64))
            assert torch.equal(sums[0:n // 2 if not equal else n:2], torch.full((b_,), 4.5 * (b_ - 1), dtype=F64))
            if not equal:
                assert float(sums[(n // 2 + 1) // 2 * 2::2].abs().max()) == 0.0 and a > b_
            assert torch.equal(sm_oracle.sm_matrix(corr, 0.10).to(F64), M)             # exact in fp32 too
            v = S.sm_power64(M, 1)
            want = torch.zeros(n)
            if equal:
                want[: n // 4] = 1
            else:
                want[1:2 * (n // 4):2] = 1
            assert torch.equal(S.sm_select(v, n // 4), want) and int(want.sum()) == n // 4
    for kind in ("nan", "inf"):
        corr, _, _ = S.nonfinite_case(kind)
        v32 = S.sm_power(sm_oracle.sm_matrix(corr, 0.10), 10)                          # the reference's lines: everything is NaN
        assert bool(torch.isnan(v32).all()) and bool(torch.isnan(S.sm_power64(S.sm_matrix64(corr, 0.10), 1)).all())
        assert int(torch.isnan(corr).sum()) == 1 and int((~torch.isfinite(corr)).sum()) == (1 if kind == "nan" else 65)
    corr, _, _ = S.nonfinite_case("inf entry")                                        # one inf entry alone: a zero row and column, no NaN
    M32, M64 = sm_oracle.sm_matrix(corr, 0.10), S.sm_matrix64(corr, 0.10)
    assert float(M64[33].abs().max()) == 0.0 and float(M64[:, 33].abs().max()) == 0.0 and float(M32[33].abs().max()) == 0.0
    v64 = S.sm_power64(M64, 10)
    e32 = S.err(S.sm_power(M32, 10), v64)
    assert bool(torch.isfinite(v64).all()) and float(v64[33]) == 0.0 and e32 < S.E32_MAX
    assert int(S.undecided(v64, 6, S.bound(e32) * float(v64.max())).sum()) == 0


def test_cal_confidence_input_conditions():
    """Every asserted confidence has a yardstick within 1e-3 of fp64 -- except the ratio of the recorded ill-conditioned inputs
    (spectral_oracle.CC_ILL: an input whose yardstick misses at any step count), which the GPU test then does not assert.  |v| = 3 gives a ratio near -0.125 (lambda1 - 9 lambda1 = -8 lambda1 dominates B), unit v a
    positive one: a kernel that assumed |v| = 1 cannot pass both."""
    ill = set()
    for n, symmetric, vscale, method, it in S.cc_cases():
        c64, e32 = S.cc_reference(n, symmetric, vscale, method, it)
        print(f"CC N={n} sym={symmetric} |v|={vscale} {method} iters={it}: conf64 {c64:.6e}  e32 {e32:.2e}")
        if method == "eig_value_ratio":
            if not e32 < S.E32_MAX:
                ill.add((n, symmetric, vscale))
            elif vscale == 3.0 and it == 10 and n >= 16:
                assert -0.2 < c64 < -0.1
            elif vscale == 1.0 and it == 10 and n >= 16:
                assert c64 > 0
        else:
            assert e32 < S.E32_MAX and c64 > 0
    print("ill-conditioned ratio inputs:", sorted(ill))
    assert ill == S.CC_ILL


def _eval_calls():
    """name -> (trans, gt, pred, gt_labels, re_thre, te_thre): the calls of the GPU part."""
    T, G = S.pose_rows()
    p63, l63 = S.label_rows(63)
    calls = {"poses": (T, G, p63[torch.arange(16) % 4], l63[torch.arange(16) % 4], S.RE_THRE, S.TE_THRE),
             "re_thre 0": (T[:3], G[:3], p63[:3], l63[:3], 0.0, S.TE_THRE), "te_thre 0": (T[:3], G[:3], p63[:3], l63[:3], S.RE_THRE, 0.0)}
    for n in S.EVAL_SIZES:
        p, l_ = S.label_rows(n)
        calls[f"labels N={n}"] = (T[12:16], G[12:16], p, l_, S.RE_THRE, S.TE_THRE)
    return calls


_EVAL_REF = {}


def _eval_ref(name):
    if name not in _EVAL_REF:
        a = _eval_calls()[name]
        _EVAL_REF[name] = (a, S.eval_row64(*a), S.eval_row(*a, dtype=torch.float32))
    return _EVAL_REF[name]


def test_eval_inputs_are_what_they_claim():
    a, ref, yard = _eval_ref("poses")
    row = {k: i for i, k in enumerate(S.POSE_ROWS)}
    for k in ("identity", "permutation", "trace above 3"):
        assert float(ref[row[k], 1]) == 0.0 and float(ref[row[k], 2]) == 0.0 and float(ref[row[k], 0]) == 1.0
        assert float(yard[row[k], 1]) == 0.0 and float(yard[row[k], 2]) == 0.0
    R = a[0][row["trace above 3"], :3, :3]
    assert float((R.to(F64) ** 2).sum()) > 3 + 2.0 ** -22 and float((R * R).sum()) > 3.0
    # (1e-4 rad moves the trace by 1e-8, below the rounding of the fp32 entries: the row sits at the flat end of acos, inside its floor)
    assert abs(float(ref[row["1e-4 rad"], 1]) - math.degrees(1e-4)) < float(S.re_floor_deg(a[0], a[1])[row["1e-4 rad"]])
    assert abs(float(ref[row["180 deg"], 1]) - 180.0) < 1e-3
    # either side of each threshold by more than the bound of that row
    b_re = torch.maximum(4 * (yard[:, 1] - ref[:, 1]).abs(), S.re_floor_deg(a[0], a[1]))
    b_te = torch.maximum(4 * (yard[:, 2] - ref[:, 2]).abs(), S.TE_FLOOR_REL * ref[:, 2])
    for k, col, thre, b_, side in (("RE below", 1, S.RE_THRE, b_re, -1), ("RE above", 1, S.RE_THRE, b_re, 1),
                                   ("TE below", 2, S.TE_THRE, b_te, -1), ("TE above", 2, S.TE_THRE, b_te, 1)):
        margin = side * (float(ref[row[k], col]) - thre)
        print(f"{k}: {float(ref[row[k], col]):.6f} against {thre}, bound {float(b_[row[k]]):.2e}")
        assert margin > float(b_[row[k]]) and float(ref[row[k], 0]) == (1.0 if side < 0 else 0.0)
    assert math.isnan(float(ref[row["NaN rotation"], 1])) and float(ref[row["NaN rotation"], 0]) == 0.0
    assert math.isnan(float(ref[row["NaN translation"], 2])) and float(ref[row["NaN translation"], 0]) == 0.0
    assert not math.isnan(float(ref[row["NaN translation"], 1])) and int(torch.isnan(ref).sum()) == 2
    for name in ("re_thre 0", "te_thre 0"):                       # strict '<': a zero threshold is never met, not even by identical poses
        assert _eval_ref(name)[1][:, 0].tolist() == [0.0, 0.0, 0.0]
    for n in S.EVAL_SIZES:
        (_, _, pred, gtl, _, _), ref, _ = _eval_ref(f"labels N={n}")
        lab = {k: i for i, k in enumerate(S.LABEL_ROWS)}
        assert float(ref[lab["nothing predicted"], 6]) == 0.0 and float(ref[lab["no ground truth"], 7]) == 0.0
        assert ref[lab["both empty"], 5:].tolist() == [0.0, 0.0, 0.0, 0.0]
        assert int(ref[0, 3]) == int(gtl[0].sum()) and torch.equal(pred[0] > 0, (pred[0] == 0.3) | (pred[0] == 7.0))
        if n >= 63:
            vals = pred[0]
            assert all(bool((vals == x).any()) for x in (0.3, 7.0, -1.0)) and bool(torch.isnan(vals).any())
            assert bool(((vals == 0) & torch.signbit(vals)).any()) and bool(((vals == 0) & ~torch.signbit(vals)).any())
            assert 0 < int(ref[0, 5]) < int(ref[0, 3])


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: deliberate defects, applied to the fp32 yardstick -- the check has to reject each
# ---------------------------------------------------------------------------------------------------------------------------
SM_DEFECTS = [("diagonal kept", 257, "indoor", 1), ("diagonal kept", 1027, "outdoor", 1), ("ragged group dropped", 1027, "indoor", 1),
              ("ragged group dropped", 1025, "outdoor", 10), ("norm block missing", 257, "indoor", 10), ("norm block missing", 15, "outdoor", 1),
              ("buffer parity", 257, "indoor", 2), ("buffer parity", 1024, "outdoor", 1)]


@pytest.mark.parametrize("defect,n,regime,it", SM_DEFECTS)
def test_sm_eigenvector_check_rejects_deliberate_defects(defect, n, regime, it):
    c = S.sm_case(n, regime)
    M32 = sm_oracle.sm_matrix(c["corr"], c["thr"])
    if defect == "diagonal kept":
        M32 = M32 + 4.5 * torch.eye(n)
    moved = S.err(S.sm_power(M32, it, defect), c["v64"][it])
    print(f"{defect}, N={n} {regime} iters={it}: err {moved:.2e}, bound of the case {c['bound'][it]:.2e}")
    assert moved > 10 * c["bound"][it]


def test_sm_label_check_rejects_the_descending_tie_rule():
    for n in (40, 300):
        for equal in (False, True):
            v32 = S.sm_power(sm_oracle.sm_matrix(S.tie_case(n, equal), 0.10), 1)
            want = S.sm_select(S.sm_power64(S.sm_matrix64(S.tie_case(n, equal), 0.10), 1), n // 4)
            assert torch.equal(S.sm_select(v32, n // 4), want)
            assert not torch.equal(S.sm_select(v32, n // 4, "tie rule descending"), want)


CC_DEFECTS = [("v normalised", True, 3.0, ("xMx", "eig_value_ratio")), ("transposed", False, 1.0, ("eig_value_ratio",)),
              ("padding", True, 1.0, S.CC_METHODS), ("padding", False, 3.0, S.CC_METHODS)]


@pytest.mark.parametrize("defect,symmetric,vscale,methods", CC_DEFECTS)
def test_cal_confidence_check_rejects_deliberate_defects(defect, symmetric, vscale, methods):
    """The Rayleigh quotient does not see |v| and neither v^T M v form sees a transpose: those defects are caught by the other methods."""
    for n in (17, 257):
        M, v = S.cc_inputs(n, symmetric, vscale)
        for method in methods:
            for it in (S.CC_RATIO_ITERS if method == "eig_value_ratio" else (0,)):
                if defect == "transposed" and it != 1:     # x^T B x = x^T B^T x, and B^T has B's eigenvalues: a transpose shows through
                    continue                               # the power steps alone and fades as they converge -- hence the 1-step cases
                c64, e32 = S.cc_reference(n, symmetric, vscale, method, it)
                if defect == "padding":
                    bad = S.cal_confidence(*S.cc_padded(M, v, 8), method, it, torch.float32)
                    if method == "xMx":                    # (the formula divides by the matrix's size: the caller's N stays)
                        bad = bad * (n + 8) / n
                else:
                    bad = S.cal_confidence(M, v, method, it, torch.float32, defect)
                moved = abs(bad - c64) / abs(c64)
                print(f"{defect}, N={n} sym={symmetric} |v|={vscale} {method} iters={it}: err {moved:.2e}, bound {S.bound(e32):.2e}")
                assert e32 < S.E32_MAX and moved > 10 * S.bound(e32)


EVAL_DEFECTS = [("<=", "re_thre 0"), ("<=", "te_thre 0"), ("nan swallowed", "poses"), ("precision nan", "labels N=257"),
                ("label tail dropped", "labels N=257"), ("label tail dropped", "labels N=70001"), ("label tail dropped", "labels N=63")]


@pytest.mark.parametrize("defect,call", EVAL_DEFECTS)
def test_eval_row_check_rejects_deliberate_defects(defect, call):
    a, ref, yard = _eval_ref(call)
    assert S.check_eval(yard, ref, yard, a[0], a[1], call)[0] == []               # the yardstick itself passes
    fails, _ = S.check_eval(S.eval_row(*a, dtype=torch.float32, defect=defect), ref, yard, a[0], a[1], f"{call} with '{defect}'")
    print(fails)
    assert fails


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: argument checks before any HIP call
# ---------------------------------------------------------------------------------------------------------------------------
def test_spectral_argument_checks_on_cpu(built_lib):
    lib, p = built_lib, C.c_void_p(16)
    sm = lambda n, top, it: lib.pdsc_sm_baseline(p, p, p, 0.1, top, it, p, p, p, p, 1 << 40, 1, n, None)
    smf = lambda n, top, it, form: lib.pdsc_sm_baseline_form(p, p, p, 0.1, top, it, p, p, p, p, 1 << 40, 1, n, form, None)
    for n in (40897, 65536):                               # v lives in 160 KiB - 64 bytes of LDS, round_up(N, 64) floats: N <= 40 896
        for call in (lambda: sm(n, 10, 10), lambda: smf(n, 10, 10, 1), lambda: smf(n, 10, 10, 0)):
            assert call() == -1
            msg = lib.pdsc_last_error()
            assert b"too large" in msg and b"40896" in msg, msg
    assert lib.pdsc_sm_workspace_bytes(1, 40896) > 0
    for args in ((1, 0, 10), (100, 10, 0), (100, 101, 10), (100, -1, 10)):
        assert sm(*args) == -1 and smf(*args, 1) == -1
    assert smf(100, 10, 10, 3) == -1 and b"form=3" in lib.pdsc_last_error()
    assert smf(100, 10, 10, -1) == -1
    assert lib.pdsc_sm_baseline(None, p, p, 0.1, 10, 10, p, p, p, p, 1 << 40, 1, 100, None) == -1 and b"null pointer" in lib.pdsc_last_error()
    assert lib.pdsc_sm_baseline(p, p, p, 0.1, 10, 10, p, p, p, p, 16, 1, 100, None) == -2 and b"workspace" in lib.pdsc_last_error()
    cc = lambda ld, n, method, it=10: lib.pdsc_cal_confidence(p, ld, p, method, it, p, p, 1 << 40, 1, n, None)
    assert cc(96, 100, 0) == -1 and b"ld=96" in lib.pdsc_last_error()              # ld < N
    assert cc(102, 100, 0) == -1 and b"multiple of 4" in lib.pdsc_last_error()
    assert cc(100, 100, 3) == -1 and b"method=3" in lib.pdsc_last_error()
    assert cc(100, 100, 1, -1) == -1 and cc(100, 0, 0) == -1
    assert cc(40960, 40000, 0) == -1 and b"too large" in lib.pdsc_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: SM
# ---------------------------------------------------------------------------------------------------------------------------
def _sm(corr, src, tgt, thr, ratio, it, form="streaming"):
    from pointdsc_amd import baselines
    return baselines.SM(corr, src, tgt, thr, top_ratio=ratio, num_iterations=it, return_eig=True, form=form)


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _equal_nan_as_nan(a, b):
    return all(torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("n,regime", SM_CASES, ids=SM_IDS)
def test_sm_streaming_form_matches_fp64(n, regime):
    """Eigenvector, labels and pose of one pair at 1, 2 (N <= 300) and 10 iterations and top_ratio 0, 0.1 and 1.  With one iteration the
    eigenvector is the normalised row sums of M: the matrix kernel on its own (a kept diagonal adds 4.5 to every row sum).
    Labels equal sm_select(v64) on every decided entry; the pose is ops.rigid_transform_3d of the returned eig * labels bit for bit
    (num_top = 0 and the all-zero matrix included) and, where the labels are the oracle's and N >= 63, lies within the bound of the fp64 pose."""
    from pointdsc_amd import ops
    c = S.sm_case(n, regime)
    corr, src, tgt = g(c["corr"][None]), g(c["src"][None]), g(c["tgt"][None])
    for it in S.sm_iters(n):
        v64, b = c["v64"][it], c["bound"][it]
        mx = float(v64.abs().max())
        for ratio in S.SM_TOP_RATIOS:
            num_top = int(n * ratio)
            trans, labels, eig = _sm(corr, src, tgt, c["thr"], ratio, it)
            assert _bits_equal([trans], [ops.rigid_transform_3d(src, tgt, eig * labels)])
            eig, labels, trans = eig[0].cpu(), labels[0].cpu(), trans[0].cpu()
            if mx == 0.0:
                e = float(eig.abs().max())
                print(f"SM N={n} {regime} iters={it} top={num_top}: all-zero matrix, max|eig| {e}")
                assert e == 0.0
            else:
                e = S.err(eig, v64)
                print(f"SM N={n} {regime} iters={it} top={num_top}: e32 {c['e32'][it]:.2e}  bound {b:.2e}  eig err {e:.2e}  ratio {e / b:.3f}")
                assert e <= b
            want = S.sm_select(v64, num_top)
            und = S.undecided(v64, num_top, b * mx)
            flips = int((labels != want).sum())
            assert int(labels.sum()) == num_top and set(labels.tolist()) <= {0.0, 1.0}
            assert torch.equal(labels[~und], want[~und]) and flips <= cap(n), (flips, int(und.sum()))
            if flips == 0 and n >= 63 and num_top > 0:
                T64, T32, scale, floor = S.sm_pose_reference(c, it, want)
                e32p, ep = float((T32.to(F64) - T64).abs().max()) / scale, float((trans.to(F64) - T64).abs().max()) / scale
                bp = S.bound(e32p, floor)
                print(f"SM N={n} {regime} iters={it} top={num_top}: pose e32 {e32p:.2e}  bound {bp:.2e}  pose err {ep:.2e}  ratio {ep / bp:.3f}")
                assert ep <= bp


@pytest.mark.gpu
def test_sm_batch_of_three_equals_the_single_pair_calls():
    corr, src, tgt = (g(torch.stack([S.sm_case(257, r)[k] for r in ("indoor", "outdoor", "indoor")])) for k in ("corr", "src", "tgt"))
    corr[2], src[2], tgt[2] = corr[2].flip(0), src[2].flip(0), tgt[2].flip(0)            # a third, different pair
    for it in (1, 10):
        batch = _sm(corr, src, tgt, 0.10, 0.1, it)
        for i in range(3):
            one = _sm(corr[i:i + 1], src[i:i + 1], tgt[i:i + 1], 0.10, 0.1, it)
            assert _bits_equal([x[i:i + 1] for x in batch], one), (it, i)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (40, 300))
def test_sm_exact_ties_are_cut_by_ascending_index(n):
    """Row sums 4.5 (|A| - 1) on the odd indices, smaller ones elsewhere: num_top = N / 4 cuts inside A and keeps its first N / 4
    members; with |A| = |B| every entry ties and the indices 0 .. N / 4 - 1 are kept."""
    for equal in (False, True):
        corr = S.tie_case(n, equal)
        v64 = S.sm_power64(S.sm_matrix64(corr, 0.10), 1)
        _, labels, eig = _sm(g(corr[None]), g(corr[None, :, :3]), g(corr[None, :, 3:]), 0.10, 0.25, 1)
        e = S.err(eig[0].cpu(), v64)
        print(f"SM ties N={n} equal={equal}: eig err {e:.2e}  bound {S.FLOOR:.2e}")
        assert e <= S.FLOOR
        assert torch.equal(labels[0].cpu(), S.sm_select(v64, n // 4))
        assert labels[0].cpu().nonzero().flatten().tolist() == (list(range(n // 4)) if equal else list(range(1, 2 * (n // 4), 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("nan", "inf"))
def test_sm_nonfinite_coordinate_gives_nan_as_the_reference(kind):
    """torch.clamp(min=0) keeps the NaN of a distance difference: eigenvector and pose are NaN, the labels are sm_select's answer for
    an all-NaN vector, and the finite pairs on either side of it in a batch keep the bits of their own calls -- in both forms."""
    corr, src, tgt = S.nonfinite_case(kind)
    fin = [S.sm_case(65, r) for r in ("indoor", "outdoor")]
    C_, S_, T_ = (g(torch.stack([fin[0][k], x, fin[1][k]])) for k, x in (("corr", corr), ("src", src), ("tgt", tgt)))
    num_top = int(65 * 0.1)
    batch = _sm(C_, S_, T_, 0.10, 0.1, 10)
    for i in range(3):
        one = _sm(C_[i:i + 1], S_[i:i + 1], T_[i:i + 1], 0.10, 0.1, 10)
        assert _equal_nan_as_nan([x[i:i + 1] for x in batch], one), i
        res = _sm(C_[i:i + 1], S_[i:i + 1], T_[i:i + 1], 0.10, 0.1, 10, form="resident")
        assert _equal_nan_as_nan(res, one), i
        assert bool(torch.isnan(one[2]).all()) == (i == 1) and bool(torch.isnan(one[0][0, :3]).all()) == (i == 1)
        assert bool(torch.isfinite(one[2]).all()) == (i != 1) and bool(torch.isfinite(one[0]).all()) == (i != 1)
    trans, labels, eig = (x[1].cpu() for x in batch)
    assert torch.equal(labels, S.sm_select(torch.full((65,), float("nan")), num_top))
    assert labels.nonzero().flatten().tolist() == list(range(num_top))


@pytest.mark.gpu
def test_sm_single_inf_entry_stays_finite_as_in_the_reference():
    """One inf in corr_pos: its row and column of M are 0 and its NaN self-distance is overridden by the zero diagonal -- the NaN rule
    of the matrix kernels must come before the diagonal rule.  Eigenvector within the bound of fp64, entry 33 exactly 0, both forms."""
    from pointdsc_amd import ops
    corr, src, tgt = S.nonfinite_case("inf entry")
    v64 = S.sm_power64(S.sm_matrix64(corr, 0.10), 10)
    e32 = S.err(S.sm_power(sm_oracle.sm_matrix(corr, 0.10), 10), v64)
    c, s_, t_ = g(corr[None]), g(src[None]), g(tgt[None])
    trans, labels, eig = _sm(c, s_, t_, 0.10, 0.1, 10)
    e = S.err(eig[0].cpu(), v64)
    print(f"SM inf entry N=65: e32 {e32:.2e}  bound {S.bound(e32):.2e}  eig err {e:.2e}  ratio {e / S.bound(e32):.3f}")
    assert e <= S.bound(e32) and float(eig[0, 33]) == 0.0 and bool(torch.isfinite(trans).all())
    assert torch.equal(labels[0].cpu(), S.sm_select(v64, 6)) and int(S.undecided(v64, 6, S.bound(e32) * float(v64.max())).sum()) == 0
    assert _bits_equal([trans], [ops.rigid_transform_3d(s_, t_, eig * labels)])
    assert _bits_equal(_sm(c, s_, t_, 0.10, 0.1, 10, form="resident"), (trans, labels, eig))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (2, 17, 257, 1027))
def test_sm_resident_form_equals_the_streaming_form_at_the_edges(n):
    c = S.sm_case(n, "indoor")
    corr, src, tgt = g(c["corr"][None]), g(c["src"][None]), g(c["tgt"][None])
    for it in (1, 10):
        a, b = _sm(corr, src, tgt, c["thr"], 0.1, it, form="resident"), _sm(corr, src, tgt, c["thr"], 0.1, it)
        assert _bits_equal(a, b), it


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: cal_confidence
# ---------------------------------------------------------------------------------------------------------------------------
def _cc_matrix(M, layout, lib):
    """[N,N] -> [1,N,ld] on the device: 'round4' (the wrapper pads to a multiple of 4), 'compat' (pdsc_compat_ld, zeros) or 'nan'
    (N + 8 columns, NaN in [N, N + 8))."""
    n = M.shape[0]
    if layout == "round4":
        return g(M[None])
    ld = int(lib.pdsc_compat_ld(n)) if layout == "compat" else n + 8
    out = torch.full((1, n, ld), 0.0 if layout == "compat" else float("nan"))
    out[0, :, :n] = M
    return g(out)


@pytest.mark.gpu
@pytest.mark.parametrize("n", S.CC_SIZES)
def test_cal_confidence_matches_fp64(n, built_lib):
    """Three methods, symmetric and non-symmetric M, |v| = 1 and 3, 0 / 1 / 10 deflated power steps, three layouts of the rows -- the
    padding columns of one holding NaN."""
    from pointdsc_amd import baselines
    for symmetric in (True, False):
        for vscale in (1.0, 3.0):
            M, v = S.cc_inputs(n, symmetric, vscale)
            vd = g(v[None])
            for layout in ("round4", "compat", "nan"):
                Md = _cc_matrix(M, layout, built_lib)
                for case in S.cc_cases():
                    if case[:3] != (n, symmetric, vscale):
                        continue
                    method, it = case[3], case[4]
                    got = float(baselines.cal_confidence(Md, vd, method=method, num_iterations=it))
                    c64, e32 = S.cc_reference(*case)
                    if method == "eig_value_ratio" and (n, symmetric, vscale) in S.CC_ILL:
                        print(f"CC N={n} sym={symmetric} |v|={vscale} {layout} {method} iters={it}: ill-conditioned input (e32 {e32:.2e}), got {got:.6e}, not asserted")
                        continue
                    e, b = abs(got - c64) / abs(c64), S.bound(e32)
                    print(f"CC N={n} sym={symmetric} |v|={vscale} {layout} {method} iters={it}: conf64 {c64:.6e}  e32 {e32:.2e}  bound {b:.2e}  "
                          f"err {e:.2e}  ratio {e / b:.3f}")
                    assert e <= b


@pytest.mark.gpu
@pytest.mark.parametrize("n", (17, 257))
def test_cal_confidence_batch_of_three_different_matrices(n):
    from pointdsc_amd import baselines
    Ms, v1 = S.cc_inputs(n, True, 1.0)
    Mn, v3 = S.cc_inputs(n, False, 3.0)
    Ms_, vs_ = [Ms, Mn, Mn.t().contiguous()], [v1, v3, (v1 * 2).contiguous()]
    Md, vd = g(torch.stack(Ms_)), g(torch.stack(vs_))
    for method, it in (("eig_value", 0), ("xMx", 0), ("eig_value_ratio", 1), ("eig_value_ratio", 10)):
        got = baselines.cal_confidence(Md, vd, method=method, num_iterations=it)
        for i in range(3):
            one = baselines.cal_confidence(Md[i:i + 1], vd[i:i + 1], method=method, num_iterations=it)
            assert torch.equal(got[i:i + 1].view(torch.int32), one.view(torch.int32))
            c64 = S.cal_confidence64(Ms_[i], vs_[i], method, it)
            e32 = abs(S.cal_confidence(Ms_[i], vs_[i], method, it, torch.float32) - c64) / abs(c64)
            e, b = abs(float(got[i]) - c64) / abs(c64), S.bound(e32)
            print(f"CC batch N={n} pair {i} {method} iters={it}: e32 {e32:.2e}  bound {b:.2e}  err {e:.2e}  ratio {e / b:.3f}")
            assert e32 < S.E32_MAX and e <= b


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the eval row
# ---------------------------------------------------------------------------------------------------------------------------
def _eval_gpu(name):
    from pointdsc_amd import ops
    a, ref, yard = _eval_ref(name)
    got = ops.eval_stats(g(a[0]), g(a[1]), g(a[2]), g(a[3]), a[4], a[5]).cpu()
    fails, _ = S.check_eval(got, ref, yard, a[0], a[1], name)
    assert not fails, fails
    return got, ref


@pytest.mark.gpu
def test_eval_row_poses_match_fp64():
    """16 pairs in one call: exact zeros for identical exact poses, the clamp at a trace above 3, both sides of both thresholds, and a
    NaN rotation or translation giving a NaN entry and success 0."""
    got, ref = _eval_gpu("poses")
    row = {k: i for i, k in enumerate(S.POSE_ROWS)}
    for k in ("identity", "permutation", "trace above 3"):
        assert got[row[k], :3].tolist() == [1.0, 0.0, 0.0]
    assert math.isnan(float(got[row["NaN rotation"], 1])) and math.isnan(float(got[row["NaN translation"], 2]))
    assert got[[row["NaN rotation"], row["NaN translation"], row["RE above"], row["TE above"]], 0].tolist() == [0.0] * 4
    assert got[[row["RE below"], row["TE below"]], 0].tolist() == [1.0, 1.0]
    for name in ("re_thre 0", "te_thre 0"):
        assert _eval_gpu(name)[0][:, 0].tolist() == [0.0, 0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", S.EVAL_SIZES)
def test_eval_row_labels_match_fp64(n):
    """One, a partial, a full and two passes of the 256-thread counting loop, and a long row; nothing predicted, no ground truth, both;
    0.3 and 7 count as predicted, -0.0, 0.0, NaN and -1 do not."""
    _eval_gpu(f"labels N={n}")
