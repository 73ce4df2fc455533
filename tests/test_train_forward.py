"""The train()-mode forward (training.train_forward / TrainablePointDSC) and harness.train_epoch.

Whole model: bs 2 x N 129, two layers, synthetic weights with randomised batch-norms, sigma = 1.5 (sigma^2 = 2.25, so
raw >= 1 - 2 / 2.25 > 0 for every pair: M's clamp cannot flip between precisions; the clamp is tests/test_feature_compat_backward.py's).
Objective L = <W1, logits> + <W2, M> with fixed seeded W1, W2 -- the forward and backward without the losses (f-11's tests).
Truth: train_oracle.TorchPointDSC in fp64 on the CPU.  Error measure, per tensor X of the logits, M, every parameter gradient
(sigma's included) and every batch-norm running statistic after the call: err(X) = max|X - X64| / max|X64| (gradients that are zero
in exact arithmetic on the scale of their convolution's weight gradient).  Yardstick e32: the maximum of the same measure for the
same torch model in fp32 ON THE DEVICE.  Bound: max(4 e32, 128 2^-24).  The figures are printed before anything is asserted."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_oracle as TO  # noqa: E402

from oracle import pointdsc_oracle as O  # noqa: E402

BS, N, LAYERS, SIGMA = 2, 129, 2, 1.5


@functools.lru_cache(maxsize=None)
def setup():
    from pointdsc_amd import PointDSC, synthetic
    state = synthetic.make_state_dict(PointDSC(num_layers=LAYERS).state_dict(), seed=3)
    state["sigma"] = torch.tensor([SIGMA], dtype=torch.float32)
    data = synthetic.make_batch(BS, N, seed=40)
    gen = torch.Generator().manual_seed(13)
    return state, data, torch.randn(BS, N, generator=gen), torch.randn(BS, N, N, generator=gen)


def load(model, state):
    model.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    return model


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names_and_state_dict():
    import pointdsc_amd
    from pointdsc_amd import PointDSC, harness, training
    assert pointdsc_amd.TrainablePointDSC is training.TrainablePointDSC and pointdsc_amd.train_forward is training.train_forward
    assert pointdsc_amd.feature_similarity is training.feature_similarity and callable(harness.train_epoch)
    a, b = PointDSC(num_layers=12), training.TrainablePointDSC(num_layers=12)
    assert len(a.state_dict()) == 358 and list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    assert isinstance(b, PointDSC) and b.training
    # the oracle model carries the same names
    assert sorted(TO.TorchPointDSC(num_layers=12).state_dict()) == sorted(a.state_dict())


def test_cpu_tensors_and_wrong_modes_are_refused():
    from pointdsc_amd import PointDSC, harness, training
    _, data, _, _ = setup()
    d = {k: data[k] for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    model = training.TrainablePointDSC(num_layers=LAYERS)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        training.train_forward(model, d)
    with pytest.raises(ValueError, match="testing"):
        model(dict(d, testing=True))
    with pytest.raises(RuntimeError, match="eval"):
        PointDSC(num_layers=LAYERS)(d)                      # the plain module keeps refusing train() mode
    with pytest.raises(RuntimeError, match="train"):
        training.train_forward(model.eval(), d)
    with pytest.raises(NotImplementedError):
        harness.train_epoch(model.train(), [data], None, weights=(1.0, 1.0, 0.5))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def g(t):
    return t.to("cuda:0")


def device_forward(captured):
    def forward(model, corr_pos, src, tgt):
        res = model({"corr_pos": corr_pos, "src_keypts": src, "tgt_keypts": tgt})
        captured["res"] = res
        return res["final_labels"], res["M"]
    return forward


def oracle_tail(normed, logits, src, tgt, model):
    """Per pair: (seed hypotheses [S',4,4], votes [S']) of the oracle's tail functions in fp64 on the forward's own features and
    logits; the seed set is extended by every logit within 1e-5 of the last seed's."""
    num_seeds, k = int(N * model.ratio), min(model.k, N - 1)
    sigma, sigma_spat = model.sigma.detach().double().cpu(), model.sigma_spat.detach().double().cpu()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        per = []
        for b in range(BS):
            order = torch.sort(logits[b], descending=True, stable=True).indices
            last = logits[b][order[num_seeds - 1]]
            seeds = order[: int((logits[b] >= last - 1e-5).sum())]
            knn_idx = O.knn_of_seeds(normed[b], seeds, k)
            per.append((knn_idx, O.seed_matrices(normed[b], src[b], tgt[b], knn_idx, sigma, sigma_spat)))
        vec_all, _ = O.power_iteration(torch.cat([p[1] for p in per], dim=0), model.num_iterations)
        out, at = [], 0
        for b, (knn_idx, _) in enumerate(per):
            vec = vec_all[at:at + knn_idx.shape[0]]
            at += knn_idx.shape[0]
            w = vec / (vec.sum(-1, keepdim=True) + 1e-6)
            seed_trans = O.rigid_transform_3d(src[b][knn_idx], tgt[b][knn_idx], w)
            votes = (O.residuals(seed_trans, src[b], tgt[b]) < model.inlier_threshold).sum(-1)
            out.append((seed_trans, votes))
        return out
    finally:
        torch.set_default_dtype(old)


@pytest.mark.gpu
def test_train_forward_against_fp64_model(monkeypatch):
    from pointdsc_amd import PointDSC, training
    state, data, W1, W2 = setup()
    corr, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
    ref64 = TO.objective_run(load(TO.TorchPointDSC(num_layers=LAYERS).double(), state), corr.double(), src.double(), tgt.double(),
                             W1.double(), W2.double())
    assert float(ref64["M"].min()) >= 0.0 and float((ref64["M"] > 0).double().mean()) > 0.99      # sigma = 1.5: nothing clamps
    torch32 = load(TO.TorchPointDSC(num_layers=LAYERS), state).to("cuda:0")
    e32s = TO.errors(TO.objective_run(torch32, g(corr), g(src), g(tgt), g(W1), g(W2)), ref64)
    e32 = max(e32s.values())

    seen = {}
    real = training.feature_similarity

    def spy(normed, sigma):                                  # the forward's own normalised features, for the tail's oracle
        seen["normed"] = normed.detach().clone()
        return real(normed, sigma)
    monkeypatch.setattr(training, "feature_similarity", spy)
    model = load(training.TrainablePointDSC(num_layers=LAYERS), state).to("cuda:0")
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    got = TO.objective_run(model, g(corr), g(src), g(tgt), g(W1), g(W2), forward=device_forward(seen))
    errs = TO.errors(got, ref64)
    worst = max(errs, key=errs.get)
    print(f"train forward bs {BS} N {N} layers {LAYERS}: e32 {e32:.3e} (worst {max(e32s, key=e32s.get)}) bound {TO.bound(e32):.3e} "
          f"worst err {errs[worst]:.3e} ({worst})")
    for name in sorted(errs):
        print(f"  {name}: {errs[name]:.2e} (torch fp32: {e32s[name]:.2e})")
    for name, e in errs.items():
        assert e <= TO.bound(e32), (name, e, TO.bound(e32))
    assert set(errs) >= {"logits", "M", "grad:sigma"} and len([k for k in errs if k.startswith("buffer:")]) == 2 * 3 * LAYERS
    sd = model.state_dict()
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(tracked) == 3 * LAYERS and all(int(sd[k]) == 1 for k in tracked)

    # final_trans: no gradient, and one of the oracle tail's hypotheses with a vote within 1 of the best
    res = seen["res"]
    assert not res["final_trans"].requires_grad and res["final_labels"].requires_grad and res["M"].requires_grad
    assert res["final_trans"].shape == (BS, 4, 4) and res["M"].shape == (BS, N, N) and res["final_labels"].shape == (BS, N)
    tail = oracle_tail(seen["normed"].double().cpu(), res["final_labels"].detach().double().cpu(), src.double(), tgt.double(), model)
    for b, (seed_trans, votes) in enumerate(tail):
        d = (seed_trans - res["final_trans"][b].double().cpu()).abs().amax((-1, -2))
        j = int(d.argmin())
        print(f"  pair {b}: nearest oracle hypothesis {j} of {len(votes)} at {float(d[j]):.2e}, votes {int(votes[j])} (max {int(votes.max())})")
        assert float(d[j]) <= 1e-4 and int(votes[j]) >= int(votes.max()) - 1

    # one Adam step, then eval(): the packed weights follow the step
    before = {k: v.clone() for k, v in model.state_dict().items()}
    opt.step()
    assert not torch.equal(before["encoder.layer0.weight"], model.state_dict()["encoder.layer0.weight"])
    model.eval()
    fresh = PointDSC(num_layers=LAYERS)
    fresh.load_state_dict(model.state_dict(), strict=True)
    fresh = fresh.to("cuda:0").eval()
    d = {"corr_pos": g(corr), "src_keypts": g(src), "tgt_keypts": g(tgt)}
    with torch.no_grad():
        for extra in ({}, {"testing": True}):
            a, f = model(dict(d, **extra)), fresh(dict(d, **extra))
            assert torch.equal(a["final_trans"], f["final_trans"]) and torch.equal(a["final_labels"], f["final_labels"])
            assert (a["M"] is None and f["M"] is None) or torch.equal(a["M"], f["M"])

    # modes
    model.train()
    with pytest.raises(ValueError, match="testing"):
        model(dict(d, testing=True))
    with pytest.raises(RuntimeError, match="eval"):
        fresh.train()(d)


@pytest.mark.gpu
def test_train_epoch_learns_is_deterministic_and_skips_non_finite_steps():
    from pointdsc_amd import PointDSC, harness, synthetic, training
    state = synthetic.make_state_dict(PointDSC(num_layers=LAYERS).state_dict(), seed=5)
    batch = synthetic.make_batch(4, 256, seed=60)
    steps = 30

    def run():
        model = load(training.TrainablePointDSC(num_layers=LAYERS), state).to("cuda:0").train()
        out = harness.train_epoch(model, [batch] * steps, torch.optim.Adam(model.parameters(), lr=1e-3))
        return out, {k: v.clone() for k, v in model.state_dict().items()}

    first, sd1 = run()
    second, sd2 = run()
    print(f"train_epoch: loss {first['loss_first']:.6f} -> {first['loss_last']:.6f}, skipped {first['skipped']}; meters "
          + " ".join(f"{k} {first[k]:.4f}" for k in harness.VALIDATE_NAMES))
    assert first["steps"] == steps and first["skipped"] == 0
    assert first["loss_last"] < first["loss_first"]
    assert set(harness.VALIDATE_NAMES) <= set(first)
    assert repr(first) == repr(second) and all(torch.equal(sd1[k], sd2[k]) for k in sd1)      # bit-identical (repr: NaN meters compare)
    assert int(sd1["encoder.blocks.PointCN_layer_0.1.num_batches_tracked"]) == steps

    # a non-finite gradient (made by a hook on the gradient: no NaN goes through the kernels): the step is skipped
    model = load(training.TrainablePointDSC(num_layers=LAYERS), state).to("cuda:0").train()
    model.classification[4].bias.register_hook(lambda grad: torch.full_like(grad, float("nan")))
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    out = harness.train_epoch(model, [batch], torch.optim.Adam(model.parameters(), lr=1e-3))
    assert out["skipped"] == 1 and out["steps"] == 1
    assert all(torch.equal(params[k], v.detach()) for k, v in model.named_parameters())
