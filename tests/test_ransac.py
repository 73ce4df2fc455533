"""f-21: correspondence RANSAC on the device (pointdsc_amd.ransac, csrc/ransac.hip) against the fp64 numpy transcription of its
contract (tests/ransac_oracle.py; the contract is written out in include/pointdsc_hip.h and DESIGN.md section 8 f-21).

The oracle solves each sample with numpy.linalg.svd, the library with its Jacobi core: on a degenerate sample (a repeated index, a
near-collinear triple) the two legitimately return different poses, and one different pose moves inlier counts by whole numbers.  The
GPU tests are therefore STAGED -- each stage is checked given the device's own output of the stage before it -- and only the
well-conditioned hypotheses are compared with the foreign solver:
  1 draws          the device's DRAW_RULE against the oracle's draws fed back through samples=: bit-identical hypothesis tables
  2 hypotheses     poses against the oracle's, distinct indices and s2 >= 0.01 s1 only, |dT| <= 1e-6 (the bound tests/test_icp.py
                   applies to the same fp64 Kabsch entry); at most 10 % may be left out; every hypothesis finite
  3 scores         SCORE_RULE of the oracle on the device's poses: counts equal, sumsq within 1e-12 relative (a different order of
                   fp64 additions over <= 1000 terms); precondition: the smallest |d2 - r^2| / r^2 exceeds 1e-9
  4 selection      SELECT_RULE of the oracle on the device's table; trans, labels, fitness, inlier_rmse follow from the table
  5 end to end     labels == gt_labels inside the mask, eval_stats reports success
  6 invariance     alone == inside a ragged batch (pair_offset), run to run, graph replay, chunk-split launch == walking launch
  7 edges          nothing-wins cases return identity / zero labels / best_iter -1; the others behave as the contract says
  8 harness        RansacModel, eval_scene(solver=...), BaselineModel unchanged
Measured on the inputs below (the oracle alone, CPU): 0 label differences, RE <= 0.45 deg, TE <= 1.9 cm."""
import ctypes as C
import functools
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_oracle as RO  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
R = 0.10
SEED = 1234
# (N, inlier ratio, make_pair seed, I, ransac_n, share of the random mask or None)
CASES = {
    "n64": (64, 0.5, 1, 64, 3, None),
    "n257_n3": (257, 0.3, 2, 256, 3, None),
    "n257_n4": (257, 0.3, 2, 256, 4, None),
    "n1000": (1000, 0.2, 3, 512, 3, None),
    "n300": (300, 0.3, 4, 300, 3, None),
    "n500_masked": (500, 0.3, 5, 256, 3, 0.4),
}
POSE_BOUND = 1e-6          # tests/test_icp.py: the pose bound of the fp64 Kabsch entry against an fp64 oracle
WELL_CONDITIONED = 0.01    # s2 >= 0.01 s1
MAX_LEFT_OUT = 0.10
SUMSQ_REL = 1e-12
MIN_MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    from pointdsc_amd import synthetic
    n, ratio, seed, I, rn, share = CASES[name]
    p = synthetic.make_pair(n, inlier_ratio=ratio, seed=seed)
    mask = None if share is None else (np.random.RandomState(100 + seed).random_sample(n) < share).astype(np.float32)
    return {"src": p["src_keypts"][0].numpy(), "tgt": p["tgt_keypts"][0].numpy(), "gt_trans": p["gt_trans"][0].numpy(),
            "gt_labels": p["gt_labels"][0].numpy(), "mask": mask, "I": I, "n": rn}


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    c = case_inputs(name)
    return RO.ransac(c["src"], c["tgt"], R, c["n"], c["I"], seed=SEED, mask=c["mask"])


def g(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def device_run(src, tgt, r=R, n=3, I=256, seed=SEED, mask=None, samples=None, pair_offset=0):
    """One pair through ransac_correspondence with the table -> dict of numpy arrays."""
    from pointdsc_amd import ransac_correspondence
    trans, labels, info = ransac_correspondence(g(src)[None], g(tgt)[None], r, ransac_n=n, max_iteration=I, seed=seed,
                                                mask=None if mask is None else g(mask)[None], pair_offset=pair_offset,
                                                samples=None if samples is None else g(samples, torch.int32)[None], return_info="table")
    out = {"trans": trans[0], "labels": labels[0]}
    out.update({k: v[0] for k, v in info.items() if torch.is_tensor(v)})
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case_device(name):
    c = case_inputs(name)
    return device_run(c["src"], c["tgt"], R, c["n"], c["I"], SEED, c["mask"])


def assert_same(a, b, what=""):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the oracle and the ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_splitmix64_published_vectors():
    got = [int(v) for v in RO.splitmix64(0, np.arange(4))]
    assert got == list(RO.SPLITMIX64_SEED0), [hex(v) for v in got]


@pytest.mark.parametrize("M", [1, 3, 190, 65536])
def test_oracle_draw_positions_below_M(M):
    pos = RO.draw_positions(SEED, 7, 2000, 8, M)
    assert pos.shape == (2000, 8) and pos.min() >= 0 and pos.max() < M
    if M >= 190:
        assert len(np.unique(pos)) > min(M, 16000) * 0.5           # the draws spread over L
    np.testing.assert_array_equal(RO.draw_positions(SEED, 7, 2000, 8, M)[5], RO.draw_positions(SEED, 0, 2000 * 8, 8, M)[7 * 2000 + 5],
                                  err_msg="the counter is (b_global * I + i) * 8 + j")


def test_oracle_select_rule_on_a_hand_made_table():
    assert RO.select([3, 5, 5, 2], [0.1, 0.4, 0.3, 0.0]) == 2          # largest count, then smallest sumsq
    assert RO.select([5, 5, 5], [0.3, 0.3, 0.3]) == 0                  # all equal: the lowest iteration
    assert RO.select([5, 5, 4], [0.3, 0.3, 0.0]) == 0
    assert RO.select([0, 0, 0], [0.0, 0.0, 0.0]) == -1                 # count 0 never wins
    assert RO.select([0, 1, 0], [0.0, 0.5, 0.0]) == 1
    assert RO.select([2, 2], [0.5, np.nextafter(0.5, 0)]) == 1         # compared on sumsq itself, not on a rounded rmse


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_alone_recovers_labels_and_pose(name):
    c, o = case_inputs(name), case_oracle(name)
    inside = np.ones(len(c["src"]), bool) if c["mask"] is None else c["mask"] > 0
    np.testing.assert_array_equal(o["labels"], c["gt_labels"] * inside)
    re_deg, te_cm = RO.pose_errors(o["trans"], c["gt_trans"])
    print(f"{name}: M {o['M']} best_iter {o['best_iter']} count {o['hyp_count'][o['best_iter']]} RE {re_deg:.3f} deg TE {te_cm:.3f} cm "
          f"margin {o['margin']:.3g}")
    assert re_deg < 15.0 and te_cm < 30.0
    assert o["margin"] > MIN_MARGIN


def test_header_declares_ransac_and_library_exports_it():
    from pointdsc_amd import _lib, ransac
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    for name in ("pdsc_ransac_workspace_bytes", "pdsc_ransac_correspondence"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
    for rule in ("DRAW_RULE", "SCORE_RULE", "SELECT_RULE", "NO_REFIT_RULE"):
        assert rule in header and rule in RO.__doc__ and rule in (ROOT / "DESIGN.md").read_text()
    assert int(re.search(r"#define PDSC_RANSAC_CHUNK (\d+)", header).group(1)) == ransac.CHUNK
    lib = _lib.load()
    assert lib.pdsc_ransac_workspace_bytes(1, 1000, 1000) > 0
    assert lib.pdsc_ransac_workspace_bytes(32, 65536, 1 << 20) > 0                 # the limits the contract promises at least
    assert lib.pdsc_ransac_workspace_bytes(0, 1000, 1000) == 0 and lib.pdsc_ransac_workspace_bytes(1, 1000, 0) == 0
    # a pair's workspace needs do not shrink when the chunk-split launch is chosen (small batches)
    assert lib.pdsc_ransac_workspace_bytes(1, 5000, 5000) > lib.pdsc_ransac_workspace_bytes(1, ransac.CHUNK, 5000)


def test_raw_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers, ransac_n 2 / 9, I = 0, unsupported sizes and a short workspace: an error and nothing enqueued (no GPU needed)."""
    from pointdsc_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)                       # never dereferenced: every call below fails its argument checks
    f = lib.pdsc_ransac_correspondence
    need = lib.pdsc_ransac_workspace_bytes(1, 100, 10)

    def call(n=3, I=10, ws=need, bs=1, N=100, src=p):
        return f(src, p, None, None, None, 0.1, n, I, 0, 0, p, p, p, p, p, p, None, None, None, p, ws, bs, N, None)
    assert call(src=None) == -1 and b"null pointer" in lib.pdsc_last_error()
    assert call(n=2) == -1 and b"ransac_n=2" in lib.pdsc_last_error()
    assert call(n=9) == -1 and b"ransac_n=9" in lib.pdsc_last_error()
    assert call(I=0) == -1 and b"max_iteration=0" in lib.pdsc_last_error()
    assert call(N=0) == -1 and call(bs=0) == -1 and call(N=(1 << 22) + 1) == -1
    assert call(ws=need - 1) == -2 and b"workspace" in lib.pdsc_last_error()
    assert call(ws=0) == -2


def test_python_argument_checks_on_cpu():
    from pointdsc_amd import baselines, harness, ransac_correspondence
    s = torch.zeros(1, 10, 3)
    for n in (2, 9):
        with pytest.raises(ValueError, match="ransac_n"):
            ransac_correspondence(s, s, ransac_n=n)
    with pytest.raises(ValueError, match="max_iteration"):
        ransac_correspondence(s, s, max_iteration=0)
    with pytest.raises(RuntimeError, match="GPU"):
        ransac_correspondence(s, s)
    with pytest.raises(RuntimeError, match="GPU"):
        baselines.RANSAC(None, s, s, 0.1)
    with pytest.raises(ValueError, match="solver"):
        harness.eval_scene(None, [], solver="GCRANSAC")
    with pytest.raises(ValueError):
        harness.BaselineModel("RANSAC")                       # the baseline route of SM / PMC stays as it is


# ---------------------------------------------------------------------------------------------------------------------------
# GPU, staged
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n257_n3", "n257_masked190"])
def test_stage1_draws_match_the_oracle_rule(name):
    c = case_inputs("n257_n3")
    mask = None
    if name == "n257_masked190":
        mask = np.zeros(257, np.float32)
        mask[np.random.RandomState(7).permutation(257)[:190]] = 1.0
    M = 257 if mask is None else 190
    for offset in (0, 5):
        drawn = device_run(c["src"], c["tgt"], R, 3, 256, SEED, mask, pair_offset=offset)
        assert int(drawn["num_candidates"]) == M
        fed = device_run(c["src"], c["tgt"], R, 3, 256, SEED, mask, samples=RO.draw_positions(SEED, offset, 256, 3, M))
        assert_same(drawn, fed, f"{name} pair_offset {offset}")
    other = device_run(c["src"], c["tgt"], R, 3, 256, SEED + 1, mask)
    assert not np.array_equal(other["hyp_count"], drawn["hyp_count"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stage2_hypotheses_against_the_foreign_solver(name):
    o, d = case_oracle(name), case_device(name)
    assert np.isfinite(d["hyp_trans"]).all()                    # every hypothesis, the degenerate ones included
    with np.errstate(invalid="ignore"):
        keep = o["distinct"] & (o["sv"][:, 1] >= WELL_CONDITIONED * o["sv"][:, 0])
    left_out = 1.0 - keep.mean()
    err = float(np.abs(d["hyp_trans"][keep] - o["hyp_trans"][keep]).max())
    print(f"{name}: left out {int((~keep).sum())} of {len(keep)} ({100 * left_out:.1f} %), max |dT| {err:.3g}")
    assert left_out <= MAX_LEFT_OUT
    assert err <= POSE_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stage3_scores_given_the_device_poses(name):
    c, o, d = case_inputs(name), case_oracle(name), case_device(name)
    L = o["L"]
    count, sumsq, margin = RO.score(d["hyp_trans"], c["src"][L], c["tgt"][L], R)
    assert margin > MIN_MARGIN, margin                            # precondition: no point sits on the threshold
    np.testing.assert_array_equal(d["hyp_count"], count)
    rel = np.abs(d["hyp_sumsq"] - sumsq) / np.maximum(sumsq, 1e-300)
    print(f"{name}: margin {margin:.3g}, max relative sumsq difference {rel.max():.3g}")
    assert (rel <= SUMSQ_REL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stage4_selection_and_outputs_given_the_device_table(name):
    c, o, d = case_inputs(name), case_oracle(name), case_device(name)
    best = RO.select(d["hyp_count"], d["hyp_sumsq"])
    assert best >= 0 and int(d["best_iter"]) == best
    trans, labels, fitness, rmse = RO.outputs(c["src"], c["tgt"], o["L"], R, best, d["hyp_trans"][best], int(d["hyp_count"][best]),
                                              float(d["hyp_sumsq"][best]))
    np.testing.assert_array_equal(d["trans"], trans)               # fp32 of the winner's pose, rounded once
    np.testing.assert_array_equal(d["labels"], labels)
    assert d["labels"].sum() == d["hyp_count"][best]
    if c["mask"] is not None:
        assert not d["labels"][c["mask"] <= 0].any()
    assert int(d["num_candidates"]) == o["M"]
    assert float(d["fitness"]) == d["hyp_count"][best] / o["M"]
    assert abs(float(d["inlier_rmse"]) - rmse) <= 1e-12 * rmse


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stage5_end_to_end_labels_and_success(name):
    from pointdsc_amd import ops
    c, d = case_inputs(name), case_device(name)
    inside = np.ones(len(c["src"]), bool) if c["mask"] is None else c["mask"] > 0
    np.testing.assert_array_equal(d["labels"], c["gt_labels"] * inside)
    st = ops.eval_stats(g(d["trans"])[None], g(c["gt_trans"])[None], g(d["labels"])[None], g(c["gt_labels"])[None], 15.0, 30.0)[0].cpu().numpy()
    print(f"{name}: RE {st[1]:.3f} deg TE {st[2]:.3f} cm")
    assert st[0] == 1.0


TABLE_KEYS = ("fitness", "inlier_rmse", "best_iter", "num_candidates", "hyp_trans", "hyp_count", "hyp_sumsq")


def _batched(srcs, tgts, masks, n, I, pair_offset=0):
    from pointdsc_amd import ransac_correspondence
    trans, labels, info = ransac_correspondence([g(s) for s in srcs], [g(t) for t in tgts], R, ransac_n=n, max_iteration=I, seed=SEED,
                                                mask=None if masks is None else [g(m) for m in masks], pair_offset=pair_offset,
                                                return_info="table")
    return trans, labels, info


@pytest.mark.gpu
def test_stage6_pair_alone_equals_pair_in_a_ragged_batch():
    """N = 1000 > CHUNK and I = 1000 > 256: more than one point chunk and more than one hypothesis tile."""
    from pointdsc_amd import ransac
    big = case_inputs("n1000")
    assert len(big["src"]) > ransac.CHUNK
    others = [case_inputs("n257_n3"), case_inputs("n300")]
    order = [big, others[0], others[1], big]
    masks = [np.ones(len(x["src"]), np.float32) for x in order]
    masks[1][::3] = 0.0
    trans, labels, info = _batched([x["src"] for x in order], [x["tgt"] for x in order], masks, 3, 1000, pair_offset=10)
    for pos in (0, 2, 3):                                  # position 2: N = 300 alone is one chunk, padded to 1000 it is two
        alone = device_run(order[pos]["src"], order[pos]["tgt"], R, 3, 1000, SEED, masks[pos], pair_offset=10 + pos)
        np.testing.assert_array_equal(trans[pos].cpu().numpy(), alone["trans"])
        np.testing.assert_array_equal(labels[pos].cpu().numpy(), alone["labels"])
        for k in TABLE_KEYS:
            np.testing.assert_array_equal(info[k][pos].cpu().numpy(), alone[k], err_msg=f"position {pos} {k}")
    assert not np.array_equal(info["hyp_count"][0].cpu().numpy(), info["hyp_count"][3].cpu().numpy())     # their counters differ
    assert int(info["best_iter"][0]) >= 0 and int(info["hyp_count"][0].max()) > 100


@pytest.mark.gpu
def test_stage6_chunk_split_launch_equals_walking_launch():
    """A small batch gives every point chunk its own workgroup, a large one lets each workgroup walk all chunks: the same bits.
    bs = 256 pairs x 4 hypothesis tiles reaches the walking launch; N = 600 > CHUNK has two chunks."""
    from pointdsc_amd import ransac, ransac_correspondence, synthetic
    n, I, bs = 600, 1000, 256
    assert n > ransac.CHUNK
    p = synthetic.make_pair(n, inlier_ratio=0.3, seed=11)
    src, tgt = p["src_keypts"].cuda(), p["tgt_keypts"].cuda()
    trans, labels, info = ransac_correspondence(src.expand(bs, n, 3).contiguous(), tgt.expand(bs, n, 3).contiguous(), R, ransac_n=3,
                                                max_iteration=I, seed=SEED, return_info="table")
    for pos in (0, 255):
        a_t, a_l, a_i = ransac_correspondence(src, tgt, R, ransac_n=3, max_iteration=I, seed=SEED, pair_offset=pos, return_info="table")
        assert torch.equal(trans[pos], a_t[0]) and torch.equal(labels[pos], a_l[0])
        for k in TABLE_KEYS:
            assert torch.equal(info[k][pos], a_i[k][0]), (pos, k)
    assert int(info["hyp_count"].max()) > 100


@pytest.mark.gpu
def test_stage6_repeatable_and_graph_capturable():
    from pointdsc_amd import ransac_correspondence
    c = case_inputs("n1000")
    src, tgt = g(c["src"])[None].expand(3, -1, -1).contiguous(), g(c["tgt"])[None].expand(3, -1, -1).contiguous()
    mask = g((np.random.RandomState(3).random_sample((3, 1000)) < 0.7).astype(np.float32))
    run = lambda: ransac_correspondence(src, tgt, R, ransac_n=3, max_iteration=1000, seed=SEED, mask=mask, return_info="table")  # noqa: E731
    a, b = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in TABLE_KEYS:
        assert torch.equal(a[2][k], b[2][k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a[0], c_out[0]) and torch.equal(a[1], c_out[1])
    for k in TABLE_KEYS:
        assert torch.equal(a[2][k], c_out[2][k]), k
    c_out[0].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a[0], c_out[0])


def _nothing_won(d, n):
    np.testing.assert_array_equal(d["trans"], np.eye(4, dtype=np.float32))
    assert not d["labels"].any() and d["labels"].shape == (n,)
    assert int(d["best_iter"]) == -1 and float(d["fitness"]) == 0.0 and float(d["inlier_rmse"]) == 0.0
    assert not d["hyp_count"].any() and not d["hyp_sumsq"].any()


@pytest.mark.gpu
def test_stage7_edges_where_nothing_wins():
    c = case_inputs("n64")
    src, tgt, n = c["src"], c["tgt"], 64
    zero = np.zeros(n, np.float32)
    d = device_run(src, tgt, I=64, mask=zero)                                  # M = 0
    _nothing_won(d, n)
    assert int(d["num_candidates"]) == 0 and np.isnan(d["hyp_trans"]).all()
    two = zero.copy()
    two[[5, 9]] = 1.0
    d = device_run(src, tgt, I=64, mask=two)                                   # M = 2 < ransac_n = 3
    _nothing_won(d, n)
    assert int(d["num_candidates"]) == 2
    for r in (0.0, float("nan"), -0.1):                                          # open3d's guard: max_correspondence_distance <= 0
        _nothing_won(device_run(src, tgt, r=r, I=64), n)
    bad = np.full((64, 3), -1, np.int64)
    bad[::2] = 64                                                              # every sample invalid: positions < 0 or >= M
    d = device_run(src, tgt, I=64, samples=bad)
    _nothing_won(d, n)
    assert np.isnan(d["hyp_trans"]).all()


@pytest.mark.gpu
def test_stage7_edges_the_contract_defines():
    """M = ransac_n is NOT an early out; a repeated index goes through the Kabsch entry's rank <= 1 fallback (a finite pose that maps
    the point onto its partner: count >= 1); a NaN coordinate is never an inlier and spoils only the samples that contain it."""
    c = case_inputs("n64")
    src, tgt, gt = c["src"], c["tgt"], c["gt_labels"]
    inl = np.flatnonzero(gt > 0)
    three = np.zeros(64, np.float32)
    three[inl[:3]] = 1.0
    d = device_run(src, tgt, I=64, mask=three)                                 # M = n = 3
    o = RO.ransac(src, tgt, R, 3, 64, seed=SEED, mask=three)
    assert int(d["num_candidates"]) == 3 and np.isfinite(d["hyp_trans"]).all()
    assert int(d["best_iter"]) == RO.select(d["hyp_count"], d["hyp_sumsq"]) >= 0
    assert d["hyp_count"].max() == 3 == o["hyp_count"].max() and d["labels"].sum() == 3
    rep = np.tile(np.arange(64)[:, None], (1, 3))                              # hypothesis i = (i, i, i)
    d = device_run(src, tgt, I=64, samples=rep)
    assert np.isfinite(d["hyp_trans"]).all() and (d["hyp_count"] >= 1).all()
    assert int(d["best_iter"]) == RO.select(d["hyp_count"], d["hyp_sumsq"]) >= 0
    assert d["labels"][int(d["best_iter"])] == 1.0
    clean = case_oracle("n64")                                                 # an inlier that some sample holds, the winner's does not
    victim = next(int(i) for i in inl if (clean["samples"] == i).any() and i not in clean["samples"][clean["best_iter"]])
    for inside in (True, False):                                               # a NaN coordinate inside / outside the mask
        s2 = src.copy()
        mask = np.ones(64, np.float32)
        s2[victim, 1] = np.nan
        if not inside:
            mask[victim] = 0.0
        d = device_run(s2, tgt, I=64, mask=mask)
        o = RO.ransac(s2, tgt, R, 3, 64, seed=SEED, mask=mask)
        hit = (o["L"][o["samples"]] == victim).any(axis=1)
        assert hit.any() == inside
        np.testing.assert_array_equal(np.isnan(d["hyp_trans"]).any(axis=(1, 2)), hit)
        assert not d["hyp_count"][hit].any() and not d["hyp_sumsq"][hit].any()
        assert int(d["best_iter"]) == RO.select(d["hyp_count"], d["hyp_sumsq"]) >= 0
        expect = gt.copy()
        expect[victim] = 0.0
        np.testing.assert_array_equal(d["labels"], expect)
        assert np.isfinite(d["trans"]).all()


@pytest.mark.gpu
def test_stage7_cuda_side_argument_checks():
    from pointdsc_amd import ransac_correspondence
    s = torch.zeros(1, 10, 3, device="cuda")
    with pytest.raises(ValueError, match="samples"):
        ransac_correspondence(s, s, max_iteration=8, samples=torch.zeros(1, 8, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        ransac_correspondence(s, s, mask=torch.zeros(1, 9, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU"):
        ransac_correspondence(s, s.cpu())


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the harness route
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stage8_ransac_model_equals_direct_baseline_calls():
    from pointdsc_amd import baselines, harness
    with pytest.raises(ValueError):
        harness.BaselineModel("RANSAC")
    assert harness.BaselineModel.METHODS == ("SM", "PMC")
    model = harness.RansacModel(R)
    a, b = case_inputs("n257_n3"), case_inputs("n300")
    src, tgt = g(a["src"])[None], g(a["tgt"])[None]
    res = model({"corr_pos": None, "src_keypts": src, "tgt_keypts": tgt, "testing": True})
    t, lab = baselines.RANSAC(None, src, tgt, R)
    assert torch.equal(res["final_trans"], t) and torch.equal(res["final_labels"], lab) and lab.shape == (1, 257)
    np.testing.assert_array_equal(lab[0].cpu().numpy(), a["gt_labels"])
    srcs, tgts = [g(a["src"]), g(b["src"])], [g(a["tgt"]), g(b["tgt"])]
    res = model({"corr_pos": None, "src_keypts": srcs, "tgt_keypts": tgts, "testing": True})
    t, lab = baselines.RANSAC(None, srcs, tgts, R)
    assert torch.equal(res["final_trans"], t) and all(torch.equal(x, y) for x, y in zip(res["final_labels"], lab))
    for i in range(2):                                     # one batched call == one call per pair with its counter offset
        ti, li = baselines.RANSAC(None, srcs[i][None], tgts[i][None], R, pair_offset=i)
        assert torch.equal(res["final_trans"][i], ti[0]) and torch.equal(res["final_labels"][i], li[0])
        assert res["final_labels"][i].shape == (len(srcs[i]),)


@pytest.mark.gpu
def test_stage8_eval_scene_solver_route():
    from pointdsc_amd import PointDSC, harness, workloads
    cloud = np.load(GOLDEN / "demo_clouds_vox005.npz")["cloud_bin_0"]
    kw = dict(workloads.BASE_MODEL)
    model = PointDSC(**kw)
    model.load_state_dict(workloads.state_dict("n5000_b32", model.state_dict()))
    model = model.eval().cuda()
    pairs = list(harness.demo_pairs(cloud, 3))
    thr = kw["inlier_threshold"]
    plain = harness.eval_scene(model, pairs, inlier_threshold=thr, batch_size=3)
    svd = harness.eval_scene(model, pairs, inlier_threshold=thr, batch_size=3, solver="SVD")
    np.testing.assert_array_equal(svd[:, :9], plain[:, :9])
    np.testing.assert_array_equal(svd[:, 11], plain[:, 11])
    r1 = harness.eval_scene(model, pairs, inlier_threshold=thr, batch_size=1, solver="RANSAC")
    r3 = harness.eval_scene(model, pairs, inlier_threshold=thr, batch_size=3, solver="RANSAC")
    assert r1.shape == r3.shape == (3, 12)
    np.testing.assert_array_equal(r1[:, :9], r3[:, :9])                       # batch_size changes neither the forward nor the draws
    np.testing.assert_array_equal(r1[:, 3:5], plain[:, 3:5])                  # the input columns do not depend on the solver
    assert not np.array_equal(r3[:, 1:3], plain[:, 1:3])                      # the pose columns come from RANSAC
    ransac_rows = harness.eval_scene(harness.RansacModel(thr), pairs, inlier_threshold=thr, batch_size=1)
    ransac_rows3 = harness.eval_scene(harness.RansacModel(thr), pairs, inlier_threshold=thr, batch_size=3)
    np.testing.assert_array_equal(ransac_rows[:, :9], ransac_rows3[:, :9])
    print("solver SVD   ", plain[:, :3].tolist(), "\nsolver RANSAC", r3[:, :3].tolist(), "\nbaseline RANSAC", ransac_rows[:, :3].tolist())
