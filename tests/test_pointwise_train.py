"""The fused train-mode point-wise layer (pdsc_pointwise_train_forward / _backward, ops.pointwise_train_*, training.conv_bn_relu,
TrainablePointDSC(fused_layers=True)).

Truth, yardstick, inputs, error measure and bound: tests/pointwise_train_oracle.py (fp64 torch on the CPU; e32 = torch's fp32
modules on the device; err(X) = max|X - X64| / max|X64|, db on dW's scale; bound max(4 e32, 128 2^-24)).  Every figure is printed
before it is asserted.  Small cases (M <= 258): truth by fp64 autograd, on generator seeds whose smallest |pre-activation| is
asserted to exceed 8 x the larger absolute pre-activation error of the device and the yardstick, so that no ReLU mask bit can
differ.  Large cases (M = 4099: 65 tiles, the last with 3 rows; M = 16451: 258 tiles for the backward's 256 persistent workgroups,
so some walk two): truth by the closed form with the mask of the side that is judged (the device's own Z > 0; torch's for e32).

Figures on one MI355X (profiles/f15_pointwise_train_errors.txt): every tensor of every case at 1.6e-8 .. 5.1e-7 against a bound of
7.6e-6 or more, except M = 2, where dY is proportional to eps / (var + eps) and the fp32 rounding of Y itself decides var on the
channel with the largest gradient: dX 6.8e-5, dW 6.7e-5 against a bound of 7.2e-5 (torch's fp32: 1.8e-5, 1.5e-5 on the device,
6.9e-5, 6.7e-5 on the CPU)."""
import ctypes as C
import functools
import inspect
import os
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_train_oracle as PO  # noqa: E402
import train_oracle as TO  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("pdsc_pointwise_train_forward", "pdsc_pointwise_train_backward", "pdsc_pointwise_train_workspace_bytes")
SMALL = [(258, cin, cout, False) for cin, cout in PO.SHAPES]
OFFSET_CASE = (258, 128, 128, True)
EDGES = [(m, 128, 64, False) for m in (2, 63, 64, 65)]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names_and_signatures():
    import pointdsc_amd
    from pointdsc_amd import _lib, ops, training
    assert pointdsc_amd.conv_bn_relu is training.conv_bn_relu and "conv_bn_relu" in pointdsc_amd.__all__
    sig = inspect.signature(training.conv_bn_relu)
    assert list(sig.parameters) == ["x", "weight", "bias", "bn_weight", "bn_bias", "running_mean", "running_var", "momentum", "eps"]
    assert sig.parameters["momentum"].default == 0.1 and sig.parameters["eps"].default == 1e-5
    assert callable(ops.pointwise_train_forward) and callable(ops.pointwise_train_backward)
    for fn in (training.TrainablePointDSC.__init__, training.train_forward):
        assert inspect.signature(fn).parameters["fused_layers"].default is False
    assert inspect.signature(training.TrainablePointDSC.__init__).parameters["fused_layers"].kind is inspect.Parameter.KEYWORD_ONLY
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pointdsc_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(",")), name
        assert hasattr(lib, name)
    q = lib.pdsc_pointwise_train_workspace_bytes
    assert q(1, 128, 128) == 0 and q(258, 96, 128) == 0 and q(258, 128, 96) == 0 and q(258, 64, 128) == 0
    for cin, cout in PO.SHAPES:
        assert q(258, cin, cout) >= 5 * (2 * cout * 8 + (cout * cin + cout) * 4) and q(2, cin, cout) > 0


def test_fused_model_keeps_the_state_dict():
    from pointdsc_amd import PointDSC, training
    a, b = PointDSC(num_layers=12), training.TrainablePointDSC(num_layers=12, fused_layers=True)
    assert b.fused_layers is True and training.TrainablePointDSC(num_layers=2).fused_layers is False
    assert len(b.state_dict()) == 358 and list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    with pytest.raises(TypeError):
        training.TrainablePointDSC(6, 2, 128, 10, 0.1, 0.1, 0.1, 40, 0.1, True)      # a tenth positional argument: the flags are keyword only


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    from pointdsc_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)         # never dereferenced: every call below must return before it enqueues anything
    big = 1 << 30

    def fwd(x=p, ws=p, nbytes=big, m=258, cin=128, cout=128, mom=0.1):
        return lib.pdsc_pointwise_train_forward(x, p, p, p, p, p, p, mom, 1e-5, p, p, p, p, ws, nbytes, m, cin, cout, None)

    def bwd(x=p, outs=(p,) * 5, ws=p, nbytes=big, m=258, cin=128, cout=128):
        return lib.pdsc_pointwise_train_backward(x, p, p, p, p, p, p, p, *outs, ws, nbytes, m, cin, cout, None)
    for call in (fwd, bwd):
        assert call(x=None) == -1 and b"null pointer" in lib.pdsc_last_error()
        assert call(cout=96) == -1 and b"(128, 96)" in lib.pdsc_last_error()
        assert call(cin=64, cout=128) == -1
        assert call(m=1) == -1 and b"M=1" in lib.pdsc_last_error()
        assert call(ws=None) == -1
        assert call(x=C.c_void_p(4100)) == -1 and b"aligned" in lib.pdsc_last_error()
        need = lib.pdsc_pointwise_train_workspace_bytes(258, 128, 128)
        assert call(nbytes=need - 1) == -2 and b"workspace" in lib.pdsc_last_error()
    assert fwd(mom=1.5) == -1 and b"momentum" in lib.pdsc_last_error()
    assert bwd(outs=(None,) * 5) == -1 and b"no gradient" in lib.pdsc_last_error()


def test_conv_bn_relu_refuses_what_it_cannot_do():
    from pointdsc_amd import conv_bn_relu

    def args(m=8, cin=128, cout=64, dtype=torch.float32):
        c = PO.make_case(m, cin, cout, 1)
        return [c[k].to(dtype) for k in ("x", "w", "b", "gamma", "beta", "running_mean", "running_var")]
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv_bn_relu(*args())
    a = args()
    a[1] = a[1][:, :, None]                                   # the Conv1d's own [Cout, Cin, 1]
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv_bn_relu(*a)
    with pytest.raises(TypeError, match="torch.float32"):
        conv_bn_relu(*args(dtype=torch.float64))
    a = args()
    a[0] = a[0].half()
    with pytest.raises(TypeError, match="x must be torch.float32"):
        conv_bn_relu(*a)
    for cin, cout in ((128, 96), (64, 128), (32, 64)):
        with pytest.raises(ValueError, match="supported"):
            conv_bn_relu(*args(cin=cin, cout=cout))
    with pytest.raises(ValueError, match="at least 2"):
        conv_bn_relu(*args(m=1))
    a = args()
    a[4] = a[4][:-1]
    with pytest.raises(ValueError, match="bn_bias must be"):
        conv_bn_relu(*a)
    for i, name in ((5, "running_mean"), (6, "running_var")):
        a = args()
        a[i] = a[i].requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} gets no gradient"):
            conv_bn_relu(*a)


@pytest.mark.parametrize("key", SMALL + [OFFSET_CASE] + EDGES, ids=lambda k: f"M{k[0]}_{k[1]}x{k[2]}{'_offset' if k[3] else ''}")
def test_closed_form_equals_autograd_and_seed_margins(key):
    c64 = PO.to(PO.seeded_case(*key), torch.float64)
    ref, closed = PO.truth(*key), PO.closed_form(c64)
    errs = PO.errors(closed, ref)
    m = PO.margin(ref)
    print(f"{key}: margin {m:.3e}; closed form against autograd " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12 and float((closed["pre"] - ref["pre"]).abs().max()) <= 1e-12
    assert m > PO.MARGIN_FLOOR
    if key[3]:
        y = c64["x"] @ c64["w"].T + c64["b"]
        ratio = (y.mean(0) ** 2 / y.var(0, unbiased=False))[list(PO.OFFSET_CHANNELS)]
        assert float(ratio.min()) > 400                       # mean^2 is several hundred times the variance on the eight channels


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
EXTRA = ("y", "mean", "invstd")


def device_run(c: dict, wants=(True,) * 5) -> dict:
    """The raw ops on a case that lives on the device -> the oracle's TENSORS, 'pre', and y, mean, invstd.  c's running statistics
    are updated in place (they are the result's)."""
    from pointdsc_amd import ops
    z, y, mean, invstd = ops.pointwise_train_forward(c["x"], c["w"], c["b"], c["gamma"], c["beta"], c["running_mean"], c["running_var"],
                                                     PO.MOMENTUM, PO.EPS)
    dx, dw, db, dgamma, dbeta = ops.pointwise_train_backward(c["x"], c["w"], c["gamma"], c["beta"], y, mean, invstd, c["dz"], *wants)
    # z IS the pre-activation where it is positive; elsewhere the forward's fp32 expression on the fp32 roundings of the statistics
    pre = torch.where(z > 0, z, c["gamma"] * ((y - mean.float()) * invstd.float()) + c["beta"])
    return {"z": z, "pre": pre, "running_mean": c["running_mean"], "running_var": c["running_var"], "dx": dx, "dw": dw, "db": db,
            "dgamma": dgamma, "dbeta": dbeta, "y": y, "mean": mean, "invstd": invstd}


def report(title, errs, e32s):
    e32 = max(e32s.values())
    print(f"{title}: e32 {e32:.3e} bound {PO.bound(e32):.3e}")
    for name in PO.TENSORS:
        print(f"  {name}: {errs[name]:.2e} (torch fp32: {e32s[name]:.2e})")
    return PO.bound(e32)


def check_small(key):
    case, ref = PO.seeded_case(*key), PO.truth(*key)
    y32 = PO.autograd_run(PO.to(case, device=DEV))
    got = device_run(PO.to(case, device=DEV))
    errs, e32s = PO.errors(got, ref), PO.errors(y32, ref)
    bound = report(f"pointwise train {key}", errs, e32s)
    margin, pe, pe32 = PO.margin(ref), PO.pre_error(got, ref), PO.pre_error(y32, ref)
    print(f"  smallest |pre-activation| {margin:.3e}; absolute pre-activation error: device {pe:.2e}, torch fp32 {pe32:.2e}")
    assert margin > 8 * max(pe, pe32)
    assert torch.equal((got["z"] > 0).cpu(), ref["pre"] > 0)
    for name, e in errs.items():
        assert e <= bound, (name, e, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("key", SMALL, ids=lambda k: f"{k[1]}x{k[2]}")
def test_op_against_fp64_at_258_rows(key):
    check_small(key)


@pytest.mark.gpu
def test_large_channel_offset():
    check_small(OFFSET_CASE)


@pytest.mark.gpu
@pytest.mark.parametrize("key", EDGES, ids=lambda k: f"M{k[0]}")
def test_tile_edges(key):
    check_small(key)


@functools.lru_cache(maxsize=None)
def large_case(m: int) -> dict:
    return PO.make_case(m, 128, 128, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [4099, 16451])
def test_many_partials(m):
    case = large_case(m)
    c64 = PO.to(case, torch.float64)
    got = device_run(PO.to(case, device=DEV))
    y32 = PO.autograd_run(PO.to(case, device=DEV))
    errs = PO.errors(got, PO.closed_form(c64, (got["z"] > 0).cpu()))
    e32s = PO.errors(y32, PO.closed_form(c64, (y32["z"] > 0).cpu()))
    bound = report(f"pointwise train M {m} 128x128, closed form with each side's own mask", errs, e32s)
    for name, e in errs.items():
        assert e <= bound, (name, e, bound)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    case = large_case(4099)
    a, b = device_run(PO.to(case, device=DEV)), device_run(PO.to(case, device=DEV))
    for name in PO.TENSORS + EXTRA:
        assert torch.equal(a[name], b[name]), name


@pytest.mark.gpu
def test_optional_outputs():
    from pointdsc_amd import conv_bn_relu
    case = PO.seeded_case(258, 128, 128)
    names = ("x", "w", "b", "gamma", "beta")

    def run(need):
        c = PO.to(case, device=DEV)
        leaves = [c[k].requires_grad_(n) for k, n in zip(names, need)]
        z = conv_bn_relu(*leaves, c["running_mean"], c["running_var"], PO.MOMENTUM, PO.EPS)
        z.backward(c["dz"])
        return z.detach(), [t.grad for t in leaves]
    z_all, full = run((True,) * 5)
    raw = device_run(PO.to(case, device=DEV))
    assert torch.equal(z_all, raw["z"])
    for t, name in zip(full, ("dx", "dw", "db", "dgamma", "dbeta")):
        assert torch.equal(t, raw[name]), name               # the autograd function hands the raw op's bits through
    z, grads = run((False, True, True, True, True))
    assert grads[0] is None and torch.equal(z, z_all) and all(torch.equal(a, b) for a, b in zip(grads[1:], full[1:]))
    z, grads = run((True, False, False, False, False))
    assert all(t is None for t in grads[1:]) and torch.equal(grads[0], full[0])
    z, grads = run((False, False, False, True, True))         # no GEMM launch at all
    assert grads[:3] == [None] * 3 and torch.equal(grads[3], full[3]) and torch.equal(grads[4], full[4])
    from pointdsc_amd import ops
    c = PO.to(case, device=DEV)
    only_db = ops.pointwise_train_backward(c["x"], c["w"], c["gamma"], c["beta"], raw["y"], raw["mean"], raw["invstd"], c["dz"],
                                           False, False, True, False, False)
    assert only_db[0] is None and only_db[1] is None and torch.equal(only_db[2], raw["db"])


@pytest.mark.gpu
def test_graph_capture_replays_the_eager_bits():
    case = PO.seeded_case(258, 128, 128)
    c = PO.to(case, device=DEV)
    rm0, rv0 = c["running_mean"].clone(), c["running_var"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = {k: v.clone() for k, v in device_run(c).items()}
    side.synchronize()
    c["running_mean"].copy_(rm0)
    c["running_var"].copy_(rv0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # one chain on one stream: no parallel branches
        out = device_run(c)
    c["running_mean"].copy_(rm0)
    c["running_var"].copy_(rv0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for name in PO.TENSORS + EXTRA:
        assert torch.equal(out[name], eager[name]), name


@pytest.mark.gpu
def test_abi_rejections_enqueue_nothing():
    from pointdsc_amd import _lib, ops
    lib = _lib.load()
    m, cin, cout = 258, 128, 128
    c = PO.to(PO.seeded_case(m, cin, cout), device=DEV)
    SENT = -777.0

    def sentinel(*shape):
        return torch.full(shape, SENT, device=DEV)
    y, z, mean, invstd = sentinel(m, cout), sentinel(m, cout), sentinel(cout).double(), sentinel(cout).double()
    dx, dw, db, dgamma, dbeta = sentinel(m, cin), sentinel(cout, cin), sentinel(cout), sentinel(cout), sentinel(cout)
    rm0, rv0 = c["running_mean"].clone(), c["running_var"].clone()
    need = int(lib.pdsc_pointwise_train_workspace_bytes(m, cin, cout))
    ws = torch.empty(need // 8 + 1, device=DEV, dtype=torch.float64)
    p, st = ops._p, ops._stream()

    def fwd(x=c["x"], nbytes=need, m_=m, cout_=cout):
        return lib.pdsc_pointwise_train_forward(p(x), p(c["w"]), p(c["b"]), p(c["gamma"]), p(c["beta"]), p(c["running_mean"]),
                                                p(c["running_var"]), PO.MOMENTUM, PO.EPS, p(y), p(z), p(mean), p(invstd), p(ws), nbytes,
                                                m_, cin, cout_, st)

    def bwd(x=c["x"], nbytes=need, m_=m, cout_=cout):
        return lib.pdsc_pointwise_train_backward(p(x), p(c["w"]), p(c["gamma"]), p(c["beta"]), p(y), p(mean), p(invstd), p(c["dz"]),
                                                 p(dx), p(dw), p(db), p(dgamma), p(dbeta), p(ws), nbytes, m_, cin, cout_, st)
    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(cout_=96) == -1 and call(m_=1) == -1
        assert call(nbytes=need - 1) == -2 and b"workspace" in lib.pdsc_last_error()
    torch.cuda.synchronize()
    for t in (y, z, mean, invstd, dx, dw, db, dgamma, dbeta):
        assert bool((t == SENT).all())
    assert torch.equal(c["running_mean"], rm0) and torch.equal(c["running_var"], rv0)
    assert fwd() == 0 and bwd() == 0                          # and the same pointers are accepted
    torch.cuda.synchronize()
    assert not bool((z == SENT).any()) and not bool((dx == SENT).any()) and not bool((dw == SENT).any())


@pytest.mark.gpu
def test_whole_model_with_fused_layers(monkeypatch):
    import test_train_forward as TF
    from pointdsc_amd import PointDSC, training
    state, data, W1, W2 = TF.setup()
    g = TF.g
    corr, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
    ref64 = TO.objective_run(TF.load(TO.TorchPointDSC(num_layers=TF.LAYERS).double(), state), corr.double(), src.double(), tgt.double(),
                             W1.double(), W2.double())
    torch32 = TF.load(TO.TorchPointDSC(num_layers=TF.LAYERS), state).to(DEV)
    e32s = TO.errors(TO.objective_run(torch32, g(corr), g(src), g(tgt), g(W1), g(W2)), ref64)
    e32 = max(e32s.values())

    calls = []
    real = training.conv_bn_relu

    def spy(*args, **kwargs):
        calls.append(tuple(args[0].shape))
        return real(*args, **kwargs)
    monkeypatch.setattr(training, "conv_bn_relu", spy)
    model = TF.load(training.TrainablePointDSC(num_layers=TF.LAYERS, fused_layers=True), state).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    seen = {}
    got = TO.objective_run(model, g(corr), g(src), g(tgt), g(W1), g(W2), forward=TF.device_forward(seen))
    errs = TO.errors(got, ref64)
    worst = max(errs, key=errs.get)
    print(f"fused train forward bs {TF.BS} N {TF.N} layers {TF.LAYERS}: e32 {e32:.3e} (worst {max(e32s, key=e32s.get)}) "
          f"bound {TO.bound(e32):.3e} worst err {errs[worst]:.3e} ({worst})")
    for name in sorted(errs):
        print(f"  {name}: {errs[name]:.2e} (torch fp32: {e32s[name]:.2e})")
    assert len(calls) == 3 * TF.LAYERS and set(calls) == {(TF.BS * TF.N, 128), (TF.BS * TF.N, 64)}
    for name, e in errs.items():
        assert e <= TO.bound(e32), (name, e, TO.bound(e32))
    assert set(errs) >= {"logits", "M", "grad:sigma"} and len([k for k in errs if k.startswith("buffer:")]) == 2 * 3 * TF.LAYERS
    assert len([k for k in errs if k.startswith("grad:")]) == len([p for p in model.parameters() if p.requires_grad])
    sd = model.state_dict()
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(tracked) == 3 * TF.LAYERS and all(int(sd[k]) == 1 for k in tracked)

    # one Adam step, then eval(): equal to a plain PointDSC with the stepped state_dict, bit for bit
    before = model.state_dict()["encoder.blocks.PointCN_layer_0.0.weight"].clone()
    opt.step()
    assert not torch.equal(before, model.state_dict()["encoder.blocks.PointCN_layer_0.0.weight"])
    model.eval()
    fresh = PointDSC(num_layers=TF.LAYERS)
    fresh.load_state_dict(model.state_dict(), strict=True)
    fresh = fresh.to(DEV).eval()
    d = {"corr_pos": g(corr), "src_keypts": g(src), "tgt_keypts": g(tgt)}
    with torch.no_grad():
        for extra in ({}, {"testing": True}):
            a, f = model(dict(d, **extra)), fresh(dict(d, **extra))
            assert torch.equal(a["final_trans"], f["final_trans"]) and torch.equal(a["final_labels"], f["final_labels"])
            assert (a["M"] is None and f["M"] is None) or torch.equal(a["M"], f["M"])


@pytest.mark.gpu
def test_train_epoch_on_a_fused_model():
    import math
    from pointdsc_amd import PointDSC, harness, synthetic, training
    state = synthetic.make_state_dict(PointDSC(num_layers=2).state_dict(), seed=5)
    model = training.TrainablePointDSC(num_layers=2, fused_layers=True)
    model.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    model = model.to(DEV).train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batches = [synthetic.make_batch(4, 256, seed=60), synthetic.make_batch(4, 256, seed=61)]
    out = harness.train_epoch(model, batches, torch.optim.Adam(model.parameters(), lr=1e-3))
    print("train_epoch, fused layers: " + " ".join(f"{k} {out[k]:.4f}" for k in ("loss_first", "loss_last") + tuple(harness.VALIDATE_NAMES)))
    assert out["steps"] == 2 and out["skipped"] == 0
    assert math.isfinite(out["loss_first"]) and math.isfinite(out["loss_last"])
    assert all(math.isfinite(out[k]) for k in ("class_loss", "sm_loss") if k in out)
    after = model.state_dict()
    for k in after:
        if k.endswith("running_mean") or k.endswith("running_var") or (k.endswith(".weight") and "blocks" in k):
            assert not torch.equal(before[k], after[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == 2
