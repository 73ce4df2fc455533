"""The device losses (pointdsc_amd/losses.py, include/pointdsc_hip.h section f-11) against the fp64 oracle of tests/losses_oracle.py,
and the oracle against the reference's libs/loss.py.

Tolerances: the fp64 slots differ from the oracle by summation order only (rtol 1e-12); the features form of the spectral-matching
loss runs its Gram tiles in fp32 and is held to the bounds DERIVED in losses_oracle.py (delta, value_bound, dnormed_bound,
dsigma_bound), computed per case."""
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_oracle as LO  # noqa: E402

REFERENCE = Path("/root/reference")
RTOL = 1e-12
CASE_IDS = [f"N{c['n']}_bs{len(c['labels'])}" for c in LO.CASES]
CASE_SIGMA = [(i, s) for i in range(len(LO.CASES)) for s in LO.SIGMAS]
CASE_SIGMA_IDS = [f"{CASE_IDS[i]}_sigma{s}" for i, s in CASE_SIGMA]
VARIANTS = ["weight", "unbalanced", "balanced"]
assert {k for c in LO.CASES for k in c["labels"]} == {"none", "one", "all", "some"}      # every kind of label row is in the table
RECALL = {0: 100.0, 2: 0.0}      # the pose perturbations make the recall take both values (cases of one pair: 0 deg and 20 deg / 50 cm)


@functools.lru_cache(maxsize=None)
def case(i):
    return LO.make_case(LO.CASES[i], i)


def f64(t):
    return t.to(torch.float64)


def close(a, b, rtol=RTOL, atol=0.0):
    a, b = float(a), float(b)
    assert abs(a - b) <= rtol * abs(b) + atol, (a, b, abs(a - b))


@functools.lru_cache(maxsize=None)
def oracle_classification(i, variant):
    c = case(i)
    pred = f64(c["pred"]).requires_grad_(True)
    w = f64(c["weight"]) if variant == "weight" else None
    out = LO.classification(pred, f64(c["gt"]), w, balanced=variant == "balanced")
    out["loss"].backward()
    return out, pred.grad


@functools.lru_cache(maxsize=None)
def oracle_sm_features(i, sigma, balanced):
    c = case(i)
    normed = f64(c["normed"]).requires_grad_(True)
    sg = torch.tensor(sigma, dtype=torch.float32).to(torch.float64).requires_grad_(True)
    loss = LO.sm_features(normed, sg, f64(c["gt"]), balanced)
    loss.backward()
    return float(loss), normed.grad, float(sg.grad)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the inputs are what the table says, and the oracle is the reference
# ---------------------------------------------------------------------------------------------------------------------------
def _reference_losses():
    pytest.importorskip("sklearn")
    if not (REFERENCE / "libs" / "loss.py").exists():
        pytest.skip("the reference is not on this machine")
    sys.path.insert(0, str(REFERENCE))
    try:
        from libs import loss as ref_loss
    finally:
        sys.path.remove(str(REFERENCE))
    return ref_loss


@pytest.mark.parametrize("i", range(len(LO.CASES)), ids=CASE_IDS)
def test_oracle_equals_reference(i):
    ref = _reference_losses()
    c = case(i)
    pred, gt = c["pred"], c["gt"]
    for variant in VARIANTS:
        w = c["weight"] if variant == "weight" else None
        r = ref.ClassificationLoss(balanced=variant == "balanced")(pred, gt, w)
        o, _ = oracle_classification(i, variant)
        close(r["loss"], o["loss"].detach(), rtol=1e-5)
        assert r["precision"] == o["precision"] and r["recall"] == o["recall"] and r["f1"] == o["f1"]
        close(r["logit_true"], o["logit_true"], rtol=1e-5)
        close(r["logit_false"], o["logit_false"], rtol=1e-5)
    assert o["num_pos"] == float(torch.relu(gt.sum() - 1) + 1) and o["num_neg"] == float(torch.relu((1 - gt).sum() - 1) + 1)
    for sigma in LO.SIGMAS:
        M64 = LO.feature_matrix(f64(c["normed"]), float(np.float32(sigma)))
        M = M64.float()
        for balanced in (True, False):
            close(ref.SpectralMatchingLoss(balanced)(M, gt), LO.sm_matrix(f64(M), f64(gt), balanced), rtol=1e-5)
    # the closed-form class sizes are the reference's counted ones
    gm = LO.gt_matrix(f64(gt))
    P, Q = LO.class_sizes(f64(gt))
    assert torch.equal(P, torch.relu(gm.sum((-1, -2)) - 1) + 1) and torch.equal(Q, torch.relu((1 - gm).sum((-1, -2)) - 1) + 1)
    args = [c[k] for k in ("trans", "gt_trans", "src", "tgt", "pred")]
    r = ref.TransformationLoss(15, 30)(*args)
    o = LO.transformation(*(f64(a) for a in args))
    close(r[0], o[0], rtol=1e-5)
    assert float(r[1]) == o[1]
    # RE through an fp32 acos next to 1 carries sqrt(2^-23) rad ~ 0.02 deg; TE and RMSE are well conditioned
    close(r[2], o[2], rtol=1e-5, atol=0.05)
    close(r[3], o[3], rtol=1e-5, atol=1e-3)
    close(r[4], o[4], rtol=1e-5)


def test_cpu_tensors_raise_no_cpu_path():
    from pointdsc_amd import ClassificationLoss, SpectralMatchingLoss, TransformationLoss
    c = case(0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ClassificationLoss()(c["pred"], c["gt"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        SpectralMatchingLoss()(torch.zeros(1, 5, 5), c["gt"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        SpectralMatchingLoss().from_features(c["normed"], torch.ones(1), c["gt"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        TransformationLoss()(c["trans"], c["gt_trans"], c["src"], c["tgt"], c["pred"])


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def dev(t):
    return t.to("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("i", range(len(LO.CASES)), ids=CASE_IDS)
def test_classification_loss(i, variant):
    from pointdsc_amd import losses
    c = case(i)
    o, dpred_o = oracle_classification(i, variant)
    w = dev(c["weight"]) if variant == "weight" else None
    stats, dpred = losses.classification_loss_raw(dev(c["pred"]), dev(c["gt"]), w, variant == "balanced", want_grad=True)
    s = stats.cpu().tolist()
    print(f"[cls {CASE_IDS[i]} {variant}] loss {s[0]!r} oracle {float(o['loss'].detach())!r}")
    close(s[0], o["loss"].detach())
    assert s[1] == o["precision"] and s[2] == o["recall"] and s[3] == o["f1"]
    close(s[4], o["logit_true"])
    close(s[5], o["logit_false"])
    assert s[6] == o["num_pos"] and s[7] == o["num_neg"]
    rel = ((dpred.cpu() - dpred_o).abs() / dpred_o.abs()).max()
    print(f"[cls {CASE_IDS[i]} {variant}] max relative error of dpred {float(rel):.3e}, min |dpred| {float(dpred_o.abs().min()):.3e}")
    torch.testing.assert_close(dpred.cpu(), dpred_o, rtol=RTOL, atol=0)
    if c["pred"].shape[1] >= 64:
        assert float(c["pred"].max()) > 16 and float(c["pred"].min()) < -16          # the inputs reach both BCE tails
    # the module: same numbers, Python floats from one copy, fp32 loss
    mod = losses.ClassificationLoss(balanced=variant == "balanced")(dev(c["pred"]), dev(c["gt"]), w)
    assert mod["loss"].dtype == torch.float32 and mod["loss"].dim() == 0 and mod["loss"].is_cuda
    assert float(mod["loss"]) == float(np.float32(s[0]))
    assert [mod[k] for k in ("precision", "recall", "f1", "logit_true", "logit_false")] == s[1:6]
    ds = losses.ClassificationLoss(balanced=variant == "balanced")(dev(c["pred"]), dev(c["gt"]), w, device_stats=True)
    assert ds["f1"].is_cuda and ds["f1"].dtype == torch.float64 and float(ds["f1"]) == s[3]


@pytest.mark.gpu
@pytest.mark.parametrize("balanced", [True, False], ids=["balanced", "unbalanced"])
@pytest.mark.parametrize("i", range(len(LO.CASES)), ids=CASE_IDS)
def test_sm_loss_matrix(i, balanced):
    from pointdsc_amd import losses
    c = case(i)
    gen = torch.Generator().manual_seed(100 + i)
    bs, n = c["gt"].shape
    for M32 in (LO.feature_matrix(f64(c["normed"]), 1.0).float(), torch.rand(bs, n, n, generator=gen)):      # a symmetric and a general M
        M = f64(M32).requires_grad_(True)
        lo = LO.sm_matrix(M, f64(c["gt"]), balanced)
        lo.backward()
        loss, dM, pairs = losses.sm_loss_matrix_raw(dev(M32), dev(c["gt"]), balanced, want_grad=True)
        print(f"[sm matrix {CASE_IDS[i]} balanced={balanced}] loss {float(loss)!r} oracle {float(lo)!r}")
        close(loss, lo)
        torch.testing.assert_close(pairs.cpu(), LO.sm_pair_values(f64(M32), f64(c["gt"]), balanced), rtol=RTOL, atol=0)
        torch.testing.assert_close(dM.cpu(), M.grad, rtol=RTOL, atol=0)
        mod = losses.SpectralMatchingLoss(balanced)(dev(M32), dev(c["gt"]))
        assert mod.dtype == torch.float32 and mod.dim() == 0 and float(mod) == float(np.float32(float(loss)))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(LO.CASES)), ids=CASE_IDS)
def test_transformation_loss(i):
    from pointdsc_amd import losses
    c = case(i)
    args = [c[k] for k in ("trans", "gt_trans", "src", "tgt", "pred")]
    o = LO.transformation(*(f64(a) for a in args))
    out = losses.transformation_loss_raw(*(dev(a) for a in args)).cpu().tolist()
    print(f"[trans {CASE_IDS[i]}] device {out!r} oracle {o!r}")
    assert i not in RECALL or o[1] == RECALL[i]
    for k in (0, 2, 3, 4):
        close(out[k], o[k])
    assert out[1] == o[1]
    loss, recall, re, te, rmse = losses.TransformationLoss(15, 30)(*(dev(a) for a in args))
    assert isinstance(recall, float) and recall == o[1]
    assert loss.dtype == torch.float32 and loss.dim() == 0 and not loss.requires_grad
    assert [float(loss), float(re), float(te), float(rmse)] == [float(np.float32(out[k])) for k in (0, 2, 3, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("i,sigma", CASE_SIGMA, ids=CASE_SIGMA_IDS)
def test_sm_loss_features_value(i, sigma):
    from pointdsc_amd import losses, ops
    c = case(i)
    bs, n = c["gt"].shape
    normed, gt = dev(c["normed"]).reshape(bs * n, 128), dev(c["gt"])
    sg = torch.tensor([sigma], dtype=torch.float32, device="cuda:0")
    M = ops.feature_compat(normed, sg, bs, n)
    # a condition on the inputs: both sides of the lower clamp are reached
    raw, _ = LO.feature_raw(f64(c["normed"]), float(np.float32(sigma)))
    assert float((raw < 0).double().mean()) >= 0.05 and float(((raw > 0) & (raw < 1)).double().mean()) >= 0.05
    for balanced in (True, False):
        lf, _, _, pf = losses.sm_loss_features_raw(normed, sg, gt, balanced)
        lm, _, pm = losses.sm_loss_matrix_raw(M, gt, balanced)
        pf, pm = pf.clone(), pm.clone()
        o, _, _ = oracle_sm_features(i, sigma, balanced)
        print(f"[sm features {CASE_SIGMA_IDS[CASE_SIGMA.index((i, sigma))]} balanced={balanced}] features {float(lf)!r} matrix {float(lm)!r} "
              f"oracle {o!r} bound {LO.value_bound(float(np.float32(sigma))):.3e}")
        assert float(lf) == float(lm) and torch.equal(pf, pm)                       # bit for bit
        assert abs(float(lf) - o) <= LO.value_bound(float(np.float32(sigma)))


@pytest.mark.gpu
@pytest.mark.parametrize("i,sigma", CASE_SIGMA, ids=CASE_SIGMA_IDS)
def test_sm_loss_features_gradients(i, sigma):
    from pointdsc_amd import losses
    c = case(i)
    bs, n = c["gt"].shape
    s32 = float(np.float32(sigma))
    assert LO.kink_entries(f64(c["normed"]), s32, f64(c["gt"])) == 0       # a seed with such an entry is replaced, never dropped
    normed, gt = dev(c["normed"]).reshape(bs * n, 128), dev(c["gt"])
    sg = torch.tensor([sigma], dtype=torch.float32, device="cuda:0")
    for balanced in (True, False):
        _, dn_o, ds_o = oracle_sm_features(i, sigma, balanced)
        _, dn, ds, _ = losses.sm_loss_features_raw(normed, sg, gt, balanced, want_dnormed=True, want_dsigma=True)
        err = (f64(dn.cpu()).reshape(bs, n, 128) - dn_o).abs().amax(-1)
        bound = LO.dnormed_bound(f64(c["gt"]), s32, balanced, dn_o)
        ds_bound = LO.dsigma_bound(f64(c["normed"]), s32, f64(c["gt"]), balanced)
        print(f"[sm grad {CASE_SIGMA_IDS[CASE_SIGMA.index((i, sigma))]} balanced={balanced}] max row err / bound "
              f"{float((err / bound).max()):.3e}; dsigma {float(ds)!r} oracle {ds_o!r} bound {ds_bound:.3e}")
        assert bool((err <= bound).all())
        assert abs(float(ds) - ds_o) <= ds_bound
        # each gradient on its own
        _, dn1, ds1, _ = losses.sm_loss_features_raw(normed, sg, gt, balanced, want_dnormed=True)
        _, dn2, ds2, _ = losses.sm_loss_features_raw(normed, sg, gt, balanced, want_dsigma=True)
        assert ds1 is None and dn2 is None and torch.equal(dn1, dn) and torch.equal(ds2, ds)


@pytest.mark.gpu
def test_autograd_plumbing(monkeypatch):
    from pointdsc_amd import ClassificationLoss, SpectralMatchingLoss, losses
    c = case(3)
    bs, n = c["gt"].shape
    gt = dev(c["gt"])
    sg0 = torch.tensor([1.3], dtype=torch.float32, device="cuda:0")
    _, dpred = losses.classification_loss_raw(dev(c["pred"]), gt, None, True, want_grad=True)
    _, dn, ds, _ = losses.sm_loss_features_raw(dev(c["normed"]), sg0, gt, True, want_dnormed=True, want_dsigma=True)
    _, dM, _ = losses.sm_loss_matrix_raw(dev(LO.feature_matrix(f64(c["normed"]), 1.0).float()), gt, True, want_grad=True)
    pred, normed, sg = dev(c["pred"]).requires_grad_(True), dev(c["normed"]).requires_grad_(True), sg0.clone().requires_grad_(True)
    M = dev(LO.feature_matrix(f64(c["normed"]), 1.0).float()).requires_grad_(True)
    cls, sm = ClassificationLoss(True), SpectralMatchingLoss(True)
    loss = 1.0 * cls(pred, gt, device_stats=True)["loss"] + 1.0 * sm.from_features(normed, sg, gt) + 1.0 * sm(M, gt)
    loss.backward()
    assert torch.equal(pred.grad, dpred.float()) and torch.equal(normed.grad, dn) and torch.equal(sg.grad, ds.float())
    assert torch.equal(M.grad, dM.float())
    # an upstream gradient scales them
    pred.grad = None
    (3.0 * cls(pred, gt, device_stats=True)["loss"]).backward()
    assert torch.equal(pred.grad, (dpred * 3.0).float())
    # no requires_grad (or no_grad): the wrappers are asked for no gradient buffer, nothing carries a graph
    asked = []
    grads = {"classification_loss_raw": slice(1, 2), "sm_loss_matrix_raw": slice(1, 2), "sm_loss_features_raw": slice(1, 3)}

    def spy(name):
        raw = getattr(losses, name)

        def wrapped(*args, **kw):
            out = raw(*args, **kw)
            asked.append([name] + [x is not None for x in out[grads[name]]])      # which gradient buffers the call returned
            return out
        monkeypatch.setattr(losses, name, wrapped)
    for name in grads:
        spy(name)
    a = cls(dev(c["pred"]), gt, device_stats=True)["loss"]
    b = sm.from_features(dev(c["normed"]), sg0, gt)
    d = sm(M.detach(), gt)
    with torch.no_grad():
        e = sm.from_features(normed, sg, gt)
    assert asked == [["classification_loss_raw", False], ["sm_loss_features_raw", False, False], ["sm_loss_matrix_raw", False],
                     ["sm_loss_features_raw", False, False]]
    assert not (a.requires_grad or b.requires_grad or d.requires_grad or e.requires_grad)
    # only sigma requires a gradient: dsigma alone is written
    sm.from_features(dev(c["normed"]), sg, gt)
    assert asked[-1] == ["sm_loss_features_raw", False, True]


@pytest.mark.gpu
def test_determinism_and_batching():
    from pointdsc_amd import losses
    c = case(3)
    bs, n = c["gt"].shape
    normed, gt = dev(c["normed"]), dev(c["gt"])
    sg = torch.tensor([0.8], dtype=torch.float32, device="cuda:0")
    M = dev(LO.feature_matrix(f64(c["normed"]), 0.8).float())
    args = [dev(c[k]) for k in ("trans", "gt_trans", "src", "tgt", "pred")]

    def run():
        out = [*losses.classification_loss_raw(dev(c["pred"]), gt, None, True, want_grad=True)]
        lf, dn, ds, pf = losses.sm_loss_features_raw(normed, sg, gt, True, want_dnormed=True, want_dsigma=True)
        out += [lf, dn, ds, pf.clone()]
        lm, dM, pm = losses.sm_loss_matrix_raw(M, gt, True, want_grad=True)
        out += [lm, dM, pm.clone(), losses.transformation_loss_raw(*args)]
        return out
    first, second = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    for balanced in (True, False):
        pf = losses.sm_loss_features_raw(normed, sg, gt, balanced)[3].clone()
        pm = losses.sm_loss_matrix_raw(M, gt, balanced)[2].clone()
        for b in range(bs):
            lf1 = losses.sm_loss_features_raw(normed[b:b + 1].contiguous(), sg, gt[b:b + 1].contiguous(), balanced)[0]
            lm1 = losses.sm_loss_matrix_raw(M[b:b + 1].contiguous(), gt[b:b + 1].contiguous(), balanced)[0]
            assert float(lf1) == float(pf[b]) and float(lm1) == float(pm[b])


@pytest.mark.gpu
def test_graph_capture_features_form():
    from pointdsc_amd import SpectralMatchingLoss
    c = case(3)
    gt = dev(c["gt"])
    normed = dev(c["normed"]).requires_grad_(True)
    sg = torch.tensor([1.0], dtype=torch.float32, device="cuda:0", requires_grad=True)
    sm = SpectralMatchingLoss(True)

    def step():
        loss = sm.from_features(normed, sg, gt)
        gn, gs = torch.autograd.grad(loss, (normed, sg))
        return loss.detach(), gn, gs
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(eager, captured))


@pytest.mark.gpu
def test_harness_validate():
    from pointdsc_amd import PointDSC, harness, losses, synthetic
    kw = dict(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10, sigma_d=0.10, k=40,
              nms_radius=0.10)
    model = PointDSC(**kw)
    model.load_state_dict(synthetic.make_state_dict(model.state_dict(), seed=6))
    model = model.eval().to("cuda:0")
    batches = [synthetic.make_batch(2, 200, seed=40 + 2 * j, inlier_ratio=0.3) for j in range(2)]
    for balanced in (False, True):
        got = harness.validate(model, batches, balanced=balanced)
        want = {k: [] for k in harness.VALIDATE_NAMES}
        for batch in batches:
            d = {k: dev(v) for k, v in batch.items()}
            with torch.no_grad():
                res = model({k: d[k] for k in ("corr_pos", "src_keypts", "tgt_keypts")})
            logits, M = res["final_labels"].cpu(), res["M"].cpu()
            oc = LO.classification(f64(logits), f64(batch["gt_labels"]), None, balanced)
            ot = LO.transformation(f64(res["final_trans"].cpu()), f64(batch["gt_trans"]), f64(batch["src_keypts"]), f64(batch["tgt_keypts"]),
                                   f64(logits))
            vals = [float(oc["loss"]), ot[0], float(LO.sm_matrix(f64(M), f64(batch["gt_labels"]), balanced)), ot[1], ot[2], ot[3],
                    oc["precision"], oc["recall"], oc["f1"]]
            for k, v in zip(harness.VALIDATE_NAMES, vals):
                if not np.isnan(v):
                    want[k].append(v)
            # the storage-free form on the forward's own features is the matrix form on the M it returned, bit for bit
            normed = model.workspace_view("normed", 2, 200)[: 2 * 200 * 128].view(400, 128)
            lf = losses.sm_loss_features_raw(normed, model.sigma, d["gt_labels"], balanced)[0]
            lm = losses.sm_loss_matrix_raw(res["M"], d["gt_labels"], balanced)[0]
            assert float(lf) == float(lm)
        print(f"[validate balanced={balanced}] {got!r}")
        assert set(harness.VALIDATE_NAMES) <= set(got)
        for k in harness.VALIDATE_NAMES:
            if k in ("reg_recall", "precision", "recall", "f1"):
                assert got[k] == float(np.mean(want[k])), k
            else:
                close(got[k], np.mean(want[k]))
        assert got["sm_loss_features"] == got["sm_loss"]
