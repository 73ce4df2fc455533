"""Everything that goes through the 3x3 Kabsch / Jacobi core (csrc/kabsch3.h) against the bits recorded before the four copies of
that routine became one (tests/golden/kabsch_bits.npz, tools/record_kabsch_bits.py; inputs and runs: tests/kabsch_bits_cases.py).

Every assertion is exact equality of the raw bits -- no tolerance: with -ffp-contract=off and no fast-math the fp64 operation sequence
is what the source says, so a differing bit means the body took another operation or another branch.
  rigid_transform_3d  bs 12, n 8: rigid, noisy, coplanar, reflected, collinear, all points equal (H = 0), all weights zero, and a
                      weight_threshold > 0.  The collinear case is small integers about the origin, so its fp32 H is exactly of
                      rank 1 and the body takes the rank <= 1 fallback with a real u1; the two H = 0 cases take it with u1 = e_x
  solver tail         bs 2, N 64, S 4, 10 iterations, k = 8 and 20 (NB = 1, 2): seed_power_iteration + seed_transforms
                      (kabsch_batch_kernel), seed_solve (fixup_kabsch_kernel), post_refinement (refine_kernel); one seed's list is k
                      copies of one row (its fp32 H is rounding residue, about 1e-13, yet of full rank: the full-rank path), another's rows
                      have src y = z = 0 (rows 1, 2 of H exactly zero: the fallback)
  backward            seed_solve_backward on the same data, every seed with an upstream gradient: dnormed and the fp64 dsigma.  The
                      seed with the rank-1 H takes the `n2 = 0` statement of the backward's instantiation: s' = (s1, 0, 0), so its own
                      rows of dnormed and dsigma are 0 / 0 = NaN at the parent (with n2 left at 1 they would be finite), and NaN is
                      what is compared; a second run without that seed's upstream gradient pins the finite dsigma of the others
Which branch a case takes is not left to reading: tests/kabsch_bits_cases.kabsch_port is the body in Python floats, and the CPU tests
below hold the record itself to it (the exact rigid cases bit for bit, the NaN pattern of the backward).
  ICP                 the smallest fixture of tests/test_icp.py: fp64 pose, fitness and RMSE words
  normals             64 points with a planar patch and three collinear points: the fp64 normals"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kabsch_bits_cases as KC  # noqa: E402

TAIL_FORWARD = ("transforms.trans", "transforms.w", "transforms.mask", "solve.trans", "solve.w", "solve.mask", "refine.final",
                "refine.solves")
TAIL_BACKWARD = ("backward.dnormed", "backward.dsigma", "backward_rest.dnormed", "backward_rest.dsigma")


@pytest.fixture(scope="module")
def golden():
    with np.load(KC.GOLDEN) as d:
        return {name: torch.from_numpy(d[name]) for name in d.files}


def same_bits(got, golden, names=None):
    names = sorted(got) if names is None else names
    assert names
    for name in names:
        g, want = KC.bits(got[name]), golden[name]
        assert g.dtype == want.dtype and g.shape == want.shape, (name, g.dtype, want.dtype, tuple(g.shape), tuple(want.shape))
        assert torch.equal(g, want), f"{name}: {int((g != want).sum())} of {g.numel()} words differ from the record"


def test_inputs_cover_the_cases_the_record_names():
    A, B, W = KC.rigid_inputs()
    assert A.shape == B.shape == (12, 8, 3) and W.shape == (12, 8)
    assert float(A[6, :, 2].abs().max()) == 0.0 and float(A[9].abs().max()) == 0.0 and float(W[10].abs().max()) == 0.0
    assert 0 < int((W[11] < KC.RIGID_THRESHOLD).sum()) < 8
    for k in KC.TAIL_KS:
        knn = KC.tail_inputs(k)["knn"]
        assert knn.shape == (2, 4, k) and int(knn.min()) >= 0 and int(knn.max()) < KC.TAIL_N
        assert len(set(knn[KC.RANK0_SEED].tolist())) == 1
        assert all(len(set(knn[b, s].tolist())) == k for b in range(2) for s in range(4) if (b, s) != KC.RANK0_SEED)
        assert bool((KC.tail_inputs(k)["dtrans"][:, :, :3].abs().amax((-1, -2)) > 0).all())
        rows = knn[KC.RANK1_SEED].long()
        assert len(set(rows.tolist())) == k and float(KC.tail_inputs(k)["src"][KC.RANK1_SEED[0]][rows][:, 1:].abs().max()) == 0.0
    assert KC.normals_cloud().shape == (1, 64, 3)


def test_branch_of_every_rigid_case_and_the_record_of_the_exact_ones(golden):
    """kabsch_port on the kernel's fp32 covariance says which branch a case takes; RIGID_RANK1 and RIGID_ZERO have exact covariances, so
    the parent's recorded words must be the port's (the whole pose / the rotation: case 9's centroid of B is summed in another
    order) -- the record was taken on the rank <= 1 fallback, with a real u1 for RIGID_RANK1."""
    A, B, W = KC.rigid_inputs()
    for name, thr in (("rigid.T", 0.0), ("rigid.T_threshold", KC.RIGID_THRESHOLD)):
        for b in range(KC.RIGID_BS):
            H, cA, cB = KC.rigid_covariance(A[b], B[b], W[b], thr)
            T, branch = KC.kabsch_port(H, cA, cB)
            assert branch == ("rank1" if b == KC.RIGID_RANK1 else "zero" if b in KC.RIGID_ZERO else "full"), (name, b, branch)
            T32 = KC.bits(torch.tensor(T, dtype=torch.float64).to(torch.float32))
            if b == KC.RIGID_RANK1:
                assert all(float(x) == round(float(x)) for row in H for x in row) and max(abs(float(x)) for x in cA + cB) == 0.0
                assert torch.equal(T32, golden[name][b]), (name, b)
            elif b in KC.RIGID_ZERO:
                assert max(abs(float(x)) for row in H for x in row) == 0.0
                assert torch.equal(T32[:3, :3], golden[name][b][:3, :3]), (name, b)
            else:
                assert float((T32.view(torch.float32) - golden[name][b].view(torch.float32)).abs().max()) < 1e-5, (name, b)


@pytest.mark.parametrize("k", KC.TAIL_KS)
def test_record_of_the_backward_took_the_rank1_statement(golden, k):
    """Rows 1, 2 of RANK1_SEED's H are exactly zero whatever its weights (kabsch_port: the fallback, u1 = (+-1, 0, 0), u2 = e_y, so
    u3 . H v3 = 0 exactly): with the backward's n2 = 0 its s' is (s1, 0, 0) and Q_12 = 0 / 0.  The parent's record shows just that: NaN
    in dsigma and in exactly the rows of dnormed that seed names, and nothing but finite words once its upstream gradient is zero."""
    inp = KC.tail_inputs(k)
    rows = inp["knn"][KC.RANK1_SEED].long()
    w = torch.full((k,), 1.0 / k)
    H, cA, cB = KC.rigid_covariance(inp["src"][KC.RANK1_SEED[0]][rows], inp["tgt"][KC.RANK1_SEED[0]][rows], w)
    assert max(abs(float(x)) for x in H[1] + H[2]) == 0.0 and max(abs(float(x)) for x in H[0]) > 1e-3
    assert KC.kabsch_port(H, cA, cB)[1] == "rank1"
    dn = golden[f"tail_k{k}.backward.dnormed"].view(torch.float32)
    named = torch.zeros(KC.TAIL_BS, KC.TAIL_N, dtype=torch.bool)
    named[KC.RANK1_SEED[0], rows] = True
    assert bool(torch.isnan(dn[named]).all()) and bool(torch.isfinite(dn[~named]).all())
    assert bool(torch.isnan(golden[f"tail_k{k}.backward.dsigma"].view(torch.float64)).all())
    assert bool(torch.isfinite(golden[f"tail_k{k}.backward_rest.dnormed"].view(torch.float32)).all())
    assert bool(torch.isfinite(golden[f"tail_k{k}.backward_rest.dsigma"].view(torch.float64)).all())


@pytest.mark.gpu
def test_rigid_transform_3d_bits(golden):
    same_bits(KC.run_rigid(), golden)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KC.TAIL_KS)
def test_solver_tail_bits(golden, k):
    same_bits(KC.run_tail(k), golden, [f"tail_k{k}.{name}" for name in TAIL_FORWARD])


@pytest.mark.gpu
@pytest.mark.parametrize("k", KC.TAIL_KS)
def test_seed_solve_backward_bits(golden, k):
    same_bits(KC.run_tail(k), golden, [f"tail_k{k}.{name}" for name in TAIL_BACKWARD])


@pytest.mark.gpu
def test_icp_bits(golden):
    same_bits(KC.run_icp(), golden)


@pytest.mark.gpu
def test_normals_bits(golden):
    same_bits(KC.run_normals(), golden)
