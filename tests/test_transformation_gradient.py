"""The transformation loss with a gradient: pdsc_transformation_loss_grad behind losses.TransformationLoss,
TrainablePointDSC(differentiable_trans=True) and harness.train_epoch with a transformation weight.

Truth: fp64 autograd on the CPU -- libs/loss.py:56-61 written out below (`loss_formula`, with its two quirks: a pair counts only if
some probs > 0, and for bs > 1 the whole [bs,N,3] target is subtracted from each pair's warped source); for the whole model
train_oracle.TorchPointDSC extended by seed_solve_oracle.truth_trans (the oracle's tail functions) on the device's own seeds'
neighbours, iterate T and winning seed.  Yardstick e32: the same torch formulas in fp32 on the device.  Error measure and bound are
tests/test_train_forward.py's: err(X) = max|X - X64| / max|X64| per tensor, bound max(4 e32, 128 2^-24).  Figures are printed before
they are asserted."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_solve_oracle as SO  # noqa: E402
import train_oracle as TO  # noqa: E402

BS, N, LAYERS, SIGMA = 2, 129, 2, 1.5


def loss_formula(trans, src, tgt, probs):
    bs = trans.shape[0]
    loss = torch.zeros((), dtype=trans.dtype, device=trans.device)
    for i in range(bs):
        if int((probs[i] > 0).sum()) < 1:
            continue
        warp = src[i] @ trans[i, :3, :3].T + trans[i, :3, 3]
        loss = loss + ((warp - tgt) ** 2).sum(-1).mean()             # tgt is the whole [bs,N,3]: the reference's broadcast
    return loss / bs


def grad_or_zeros(loss, x):
    """d loss / d x; zeros where no pair counted (the formula's loss is then a constant without a graph)."""
    return torch.autograd.grad(loss, x)[0] if loss.requires_grad else torch.zeros_like(x)


@functools.lru_cache(maxsize=None)
def setup():
    from pointdsc_amd import PointDSC, synthetic
    state = synthetic.make_state_dict(PointDSC(num_layers=LAYERS).state_dict(), seed=3)
    state["sigma"] = torch.tensor([SIGMA], dtype=torch.float32)
    data = synthetic.make_batch(BS, N, seed=40)
    gen = torch.Generator().manual_seed(14)
    return state, data, torch.randn(BS, N, generator=gen), torch.randn(BS, N, N, generator=gen), torch.randn(BS, 3, 4, generator=gen)


def load(model, state):
    model.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    return model


def g(t):
    return t.to("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_train_epoch_takes_a_transformation_weight_from_a_model_that_enables_it():
    from pointdsc_amd import harness, losses, training
    _, data, _, _, _ = setup()
    plain = training.TrainablePointDSC(num_layers=LAYERS)
    enabled = training.TrainablePointDSC(num_layers=LAYERS, differentiable_trans=True)
    assert plain.differentiable_trans is False and enabled.differentiable_trans is True
    assert list(plain.state_dict()) == list(enabled.state_dict())
    opt = torch.optim.SGD(enabled.parameters(), lr=0.0)
    with pytest.raises(NotImplementedError, match="differentiable_trans=True"):
        harness.train_epoch(plain.train(), [data], opt, weights=(1.0, 1.0, 0.5))
    with pytest.raises(RuntimeError, match="no CPU path"):                       # past the refusal, to the forward
        harness.train_epoch(enabled.train(), [data], opt, weights=(1.0, 1.0, 0.5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        training.train_forward(enabled, {k: data[k] for k in ("corr_pos", "src_keypts", "tgt_keypts")}, differentiable_trans=True)
    trans = data["gt_trans"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.TransformationLoss()(trans, data["gt_trans"], data["src_keypts"], data["tgt_keypts"], data["gt_labels"])
    assert callable(losses.transformation_loss_grad_raw)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the loss
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bs", [1, 2])
def test_transformation_loss_gradient(bs):
    from pointdsc_amd import losses, synthetic
    data = synthetic.make_batch(bs + 1, N, seed=70)
    gen = torch.Generator().manual_seed(5)
    trans = data["gt_trans"].clone()
    trans[:, :3] += 0.05 * torch.randn(bs + 1, 3, 4, generator=gen)          # any 3x4: the loss does not ask for a rotation
    probs = torch.randn(bs + 1, N, generator=gen)
    probs[bs] = -probs[bs].abs()                                               # the last pair has no positive prob
    fn = losses.TransformationLoss()
    for label, sel in (("all pairs counted", slice(0, bs)), ("one pair without a positive prob", slice(1, bs + 1))):
        T, s, t, p = (x[sel].contiguous() for x in (trans, data["src_keypts"], data["tgt_keypts"], probs))
        gt = data["gt_trans"][sel].contiguous()
        T64 = T.double().requires_grad_(True)
        ref = loss_formula(T64, s.double(), t.double(), p)
        ref_g = grad_or_zeros(ref, T64)
        T32 = g(T).requires_grad_(True)
        y_g = grad_or_zeros(loss_formula(T32, g(s), g(t), g(p)), T32)
        Td = g(T).requires_grad_(True)
        out = fn(Td, g(gt), g(s), g(t), g(p))
        assert out[0].requires_grad and isinstance(out[1], float) and not any(o.requires_grad for o in out[2:])
        (got_g,) = torch.autograd.grad(3.0 * out[0], Td)
        if float(ref) == 0.0:                                                  # bs 1, its only pair without a positive prob
            print(f"bs {bs}, {label}: loss {float(out[0])}, max|d/dtrans| {float(got_g.abs().max())} (truth: exact zeros)")
            assert float(out[0]) == 0.0 and float(got_g.abs().max()) == 0.0 and float(ref_g.abs().max()) == 0.0
        else:
            e, e32 = SO.err(got_g / 3.0, ref_g), SO.err(y_g, ref_g)
            e_loss = abs(float(out[0]) - float(ref)) / abs(float(ref))
            print(f"bs {bs}, {label}: loss {float(out[0]):.6f} (err {e_loss:.2e})  d/dtrans err {e:.3e} (torch fp32 {e32:.3e}, "
                  f"bound {SO.bound(e32):.3e})")
            assert e_loss <= 2.0 ** -23 and e <= SO.bound(e32)
        assert float(got_g[:, 3].abs().max()) == 0.0
        if sel.stop == bs + 1:
            assert float(got_g[-1].abs().max()) == 0.0 and float(ref_g[-1].abs().max()) == 0.0
        # without a gradient asked for: today's behaviour, the same values, no graph
        plain = fn(g(T), g(gt), g(s), g(t), g(p))
        with torch.no_grad():
            quiet = fn(Td, g(gt), g(s), g(t), g(p))
        for o in (plain, quiet):
            assert not o[0].requires_grad and torch.equal(o[0], out[0].detach()) and o[1] == out[1]
            assert all(torch.equal(a, b) for a, b in zip(o[2:], out[2:]))
        dev = fn(Td, g(gt), g(s), g(t), g(p), device_stats=True)
        assert dev[0].requires_grad and all(x.dtype == torch.float64 and not x.requires_grad for x in dev[1:])


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the whole model
# ---------------------------------------------------------------------------------------------------------------------------
def spy_on(monkeypatch):
    """Records what the train-mode forward gave seed_solve (the device's own seeds' neighbours) and what it returned."""
    from pointdsc_amd import training
    seen = {}
    real = training.seed_solve

    def spy(normed, src, tgt, knn_idx, sigma, sigma_spat, num_iterations):
        out = real(normed, src, tgt, knn_idx, sigma, sigma_spat, num_iterations)
        seen.update(normed=normed.detach().clone(), knn=knn_idx.clone(), seed_trans=out.detach().clone())
        return out
    monkeypatch.setattr(training, "seed_solve", spy)
    return seen


def discrete_choices(seen, model, src, tgt):
    """(knn_idx [bs,S,k], T, best [bs]) of the device, recomputed by the stage ops on the recorded inputs (they are deterministic)."""
    from pointdsc_amd import _lib, ops
    _, mask, _ = ops.seed_power_iteration(seen["normed"], src, tgt, seen["knn"], model.sigma.detach(), model.sigma_spat, model.num_iterations)
    _lib.check(_lib.load().pdsc_conv_mask_all_pairs(ops._p(mask), BS, ops._stream()), "pdsc_conv_mask_all_pairs")
    best = ops.score_hypotheses(seen["seed_trans"], src, tgt, float(model.inlier_threshold))[1]
    return seen["knn"].cpu(), SO.chosen_T(mask.cpu().tolist()[0], model.num_iterations), best.cpu().long()


def torch_run(model, corr, src, tgt, choices, objective, tail):
    """TorchPointDSC forward + the tail on the device's choices; `objective(logits, M, final_trans [bs,3,4])` -> scalar; backward.
    -> dict as TO.objective_run's plus final_trans and the winners' conditioning."""
    knn, T, best = choices
    model.train()
    model.zero_grad()
    logits, M, normed = model(corr, src, tgt)
    trans, cond = tail(normed, model.sigma, src, tgt, knn.to(src.device), model.sigma_spat.detach(), T)
    rows = torch.arange(BS, device=src.device)
    final = trans[rows, best.to(src.device)][:, :3]
    objective(logits, M, final).backward()
    res = {"logits": logits.detach(), "M": M.detach(), "final_trans": final.detach()}
    for name, p in model.named_parameters():
        if p.requires_grad:
            res["grad:" + name] = torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()      # (the head, under the term alone)
    for name, b in model.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            res["buffer:" + name] = b.detach().clone()
    if cond is not None:
        res["cond"] = cond[rows, best]
    return res


def chain_tail(normed, sigma, src, tgt, knn, sigma_spat, T):
    return SO.chain(normed, sigma, src, tgt, knn.long(), sigma_spat, T), None


@pytest.mark.gpu
def test_whole_model_gradients_with_a_differentiable_final_trans(monkeypatch):
    from pointdsc_amd import training
    state, data, W1, W2, W3 = setup()
    corr, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
    seen = spy_on(monkeypatch)
    model = load(training.TrainablePointDSC(num_layers=LAYERS, differentiable_trans=True), state).to("cuda:0").train()
    d = {"corr_pos": g(corr), "src_keypts": g(src), "tgt_keypts": g(tgt)}
    res = model(d)
    assert res["final_trans"].requires_grad and res["final_trans"].shape == (BS, 4, 4)
    ((g(W1) * res["final_labels"]).sum() + (g(W2) * res["M"]).sum() + (g(W3) * res["final_trans"][:, :3]).sum()).backward()
    got = {"logits": res["final_labels"].detach(), "M": res["M"].detach(), "final_trans": res["final_trans"].detach()[:, :3]}
    got.update({"grad:" + n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad})
    got.update({"buffer:" + n: b.detach().clone() for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))})
    choices = discrete_choices(seen, model, g(src), g(tgt))
    print(f"device: iterate T = {choices[1]}, winners {choices[2].tolist()}")

    def objective(dt, dev):
        return lambda logits, M, final: (W1.to(dev, dt) * logits).sum() + (W2.to(dev, dt) * M).sum() + (W3.to(dev, dt) * final).sum()
    ref64 = torch_run(load(TO.TorchPointDSC(num_layers=LAYERS).double(), state), corr.double(), src.double(), tgt.double(), choices,
                      objective(torch.float64, "cpu"), SO.truth_trans)
    cond = ref64.pop("cond")
    print(f"conditioning of the winners: {cond.tolist()}")
    assert float(cond.min()) >= 0.03
    y32 = torch_run(load(TO.TorchPointDSC(num_layers=LAYERS), state).to("cuda:0"), g(corr), g(src), g(tgt), choices,
                    objective(torch.float32, "cuda:0"), chain_tail)
    e32s, errs = TO.errors(y32, ref64), TO.errors(got, ref64)
    e32 = max(e32s.values())
    worst = max(errs, key=errs.get)
    print(f"whole model, differentiable final_trans: e32 {e32:.3e} (worst {max(e32s, key=e32s.get)}) bound {TO.bound(e32):.3e} "
          f"worst err {errs[worst]:.3e} ({worst})")
    for name in sorted(errs):
        print(f"  {name}: {errs[name]:.2e} (torch fp32: {e32s[name]:.2e})")
    for name, e in errs.items():
        assert e <= TO.bound(e32), (name, e, TO.bound(e32))
    assert set(errs) >= {"logits", "M", "final_trans", "grad:sigma", "grad:encoder.layer0.weight"}

    # the default: the same three outputs bit for bit, no gradient on final_trans, nothing goes through seed_solve
    seen.clear()
    off = load(training.TrainablePointDSC(num_layers=LAYERS), state).to("cuda:0").train()
    res0 = off(d)
    assert not seen and not res0["final_trans"].requires_grad and res0["final_labels"].requires_grad and res0["M"].requires_grad
    for key in ("final_trans", "final_labels", "M"):
        assert torch.equal(res0[key].detach(), res[key].detach()), key


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: train_epoch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_train_epoch_with_a_transformation_weight(monkeypatch):
    """Three steps with weights (1, 1, 1) are finite.  One step with lr 0 leaves the gradients in place: those of (1, 1, 1) minus
    those of (1, 1, 0) are the transformation term.  Its truth: the fp64 model, tail and loss_formula on the device's choices.
    Measure per parameter: max|delta - term64| / max(max|term64|, max|total64|) -- the difference of two fp32 gradient sets carries
    the rounding of the TOTAL gradient (another accumulation order once a third branch joins), so the total's scale is the floor of
    what can be asked (biases whose gradient is zero in exact arithmetic: on their weight's scale, train_oracle.zero_grad_scales);
    yardstick e32: the term alone from the torch fp32 model on the device, on the same scale."""
    from pointdsc_amd import harness, training
    state, data, _, _, _ = setup()
    corr, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
    seen = spy_on(monkeypatch)

    def run(weights, steps, lr):
        model = load(training.TrainablePointDSC(num_layers=LAYERS, differentiable_trans=True), state).to("cuda:0").train()
        out = harness.train_epoch(model, [data] * steps, torch.optim.SGD(model.parameters(), lr=lr), weights=weights)
        return model, out, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}

    _, out, _ = run((1.0, 1.0, 1.0), 3, 1e-3)
    print("train_epoch (1, 1, 1), 3 steps: " + " ".join(f"{k} {out[k]:.5f}" for k in ("loss_first", "loss_last", "trans_loss", "class_loss", "sm_loss")))
    assert out["steps"] == 3 and out["skipped"] == 0
    assert all(torch.isfinite(torch.tensor(float(out[k]))) for k in ("loss_first", "loss_last", "trans_loss", "class_loss", "sm_loss"))

    model, one, g111 = run((1.0, 1.0, 1.0), 1, 0.0)
    choices = discrete_choices(seen, model, g(src), g(tgt))
    _, zero, g110 = run((1.0, 1.0, 0.0), 1, 0.0)
    assert abs((one["loss_first"] - zero["loss_first"]) - one["trans_loss"]) <= 1e-5 * max(1.0, abs(one["loss_first"]))

    def term(model, corr, src, tgt, tail):
        return torch_run(model, corr, src, tgt, choices, lambda logits, M, final: loss_formula(final, src, tgt, logits.detach()), tail)

    def total(model, corr, src, tgt, gt):
        def objective(logits, M, final):                     # (the losses' own truth lives in their tests; here only the scale is needed)
            bce = torch.nn.functional.binary_cross_entropy_with_logits(logits, gt)
            gtM = ((gt[:, None, :] + gt[:, :, None]) == 2).to(M.dtype)
            gtM = gtM * (1 - torch.eye(N, dtype=M.dtype))
            sm = ((M - gtM) ** 2).sum((-1, -2)) / (N * N)
            return bce + sm.mean() + loss_formula(final, src, tgt, logits.detach())
        return torch_run(model, corr, src, tgt, choices, objective, tail=SO.truth_trans)

    t64 = term(load(TO.TorchPointDSC(num_layers=LAYERS).double(), state), corr.double(), src.double(), tgt.double(), SO.truth_trans)
    assert float(t64["cond"].min()) >= 0.03
    tot64 = total(load(TO.TorchPointDSC(num_layers=LAYERS).double(), state), corr.double(), src.double(), tgt.double(), data["gt_labels"].double())
    t32 = term(load(TO.TorchPointDSC(num_layers=LAYERS), state).to("cuda:0"), g(corr), g(src), g(tgt), chain_tail)
    names = [n for n in g111 if "grad:" + n in t64]
    zero = TO.zero_grad_scales(names)        # biases whose gradient is zero in exact arithmetic: on their weight gradient's scale
    errs, e32s = {}, {}
    for n in names:
        ref, on = t64["grad:" + n], "grad:" + zero.get(n, n)
        scale = max(float(t64[on].abs().max()), float(tot64[on].abs().max()))
        errs[n] = float(((g111[n] - g110[n]).double().cpu() - ref).abs().max()) / scale
        e32s[n] = float((t32["grad:" + n].double().cpu() - ref).abs().max()) / scale
    e32 = max(e32s.values())
    worst = max(errs, key=errs.get)
    moved = sum(float(t64["grad:" + n].abs().max()) > 0 for n in names)
    print(f"train_epoch first step, (1,1,1) - (1,1,0) against the transformation term: e32 {e32:.3e} bound {TO.bound(e32):.3e} "
          f"worst err {errs[worst]:.3e} ({worst}); {moved} of {len(names)} parameters carry the term")
    for n, e in errs.items():
        assert e <= TO.bound(e32), (n, e, TO.bound(e32))
    assert moved >= len(names) // 2 and float(t64["grad:sigma"].abs().max()) > 0
    assert any(not torch.equal(g111[n], g110[n]) for n in names)
