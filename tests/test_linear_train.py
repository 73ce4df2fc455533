"""The train path's plain linears on the device (pdsc_linear_train_* / pdsc_qkv_train_* / pdsc_head_train_*, ops.*_train_*,
training.linear_rows / qkv_projection / classification_head, TrainablePointDSC(fused_linears=True)).

Truth, yardstick, inputs, error measure and bound: tests/linear_train_oracle.py (fp64 torch on the CPU; e32 = torch's fp32 F.linear /
relu / autograd on the device; err(X) = max|X - X64| / max|X64|; bound max(4 e32, 128 2^-24)).  Every figure is printed before it is
asserted.  The head's small case (M = 258) is judged against fp64 autograd on a generator seed whose smallest |pre-activation| is
asserted to exceed 8 x the larger absolute pre-activation error of the device and the yardstick; its large cases (M = 4099: 65
tiles, the last with 3 rows; M = 16451: 258 tiles for the backward's 256 persistent workgroups, so some walk two) against the closed
form with the masks of the side that is judged.  The whole-model case is tests/test_train_forward.py's on a batch seed whose fp64
ReLU pre-activations stay 3e-5 away from zero (linear_train_oracle.MODEL_BATCH_SEED says why that file's own batch cannot serve).

Figures on one MI355X: profiles/f16_linear_train_errors.txt."""
import ctypes as C
import inspect
import itertools
import os
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_train_oracle as LO  # noqa: E402
import train_oracle as TO  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("pdsc_linear_train_workspace_bytes", "pdsc_linear_train_forward", "pdsc_linear_train_backward",
         "pdsc_qkv_train_workspace_bytes", "pdsc_qkv_train_forward", "pdsc_qkv_train_backward",
         "pdsc_head_train_workspace_bytes", "pdsc_head_train_forward", "pdsc_head_train_backward")
M_SMALL, EDGES, LARGE = 258, (1, 63, 64, 65), (4099, 16451)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names_and_signatures():
    import pointdsc_amd
    from pointdsc_amd import _lib, ops, training
    for name in ("linear_rows", "qkv_projection", "classification_head"):
        assert getattr(pointdsc_amd, name) is getattr(training, name) and name in pointdsc_amd.__all__
    assert list(inspect.signature(training.linear_rows).parameters) == ["x", "weight", "bias", "residual"]
    assert inspect.signature(training.linear_rows).parameters["residual"].default is None
    assert list(inspect.signature(training.qkv_projection).parameters) == ["x", "wq", "bq", "wk", "bk", "wv", "bv"]
    assert list(inspect.signature(training.classification_head).parameters) == ["feat", "w0", "b0", "w1", "b1", "w2", "b2"]
    for fn in (training.TrainablePointDSC.__init__, training.train_forward):
        par = inspect.signature(fn).parameters["fused_linears"]
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("linear_train_forward", "linear_train_backward", "qkv_train_forward", "qkv_train_backward", "head_train_forward",
                 "head_train_backward"):
        assert callable(getattr(ops, name))
    assert LO.Q_SCALE == training.Q_SCALE
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pointdsc_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(",")), name
        assert hasattr(lib, name)
    assert lib.pdsc_version() == int(re.search(r"#define\s+PDSC_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    q = lib.pdsc_linear_train_workspace_bytes
    assert q(0, 64, 128) == 0 and q(258, 17, 128) == 0 and q(258, 0, 128) == 0 and q(258, 64, 96) == 0 and q(258, 128, 128) == 0
    for cin in (1, 3, 6, 16, 64):
        assert q(258, cin, 128) >= 5 * (128 * cin + 128) * 4 and q(1, cin, 128) > 0
    for q in (lib.pdsc_qkv_train_workspace_bytes, lib.pdsc_head_train_workspace_bytes):
        assert q(0) == 0 and q(-3) == 0 and q(1) > 0 and q(16451) == q(256 * 64) > q(258)      # 256 workgroups at the most


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    from pointdsc_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)         # never dereferenced: every call below must return before it enqueues anything
    big = 1 << 30

    def lin_fwd(x=p, m=258, cin=64, cout=128, **_):
        return lib.pdsc_linear_train_forward(x, p, p, p, p, m, cin, cout, None)

    def lin_bwd(x=p, outs=(p,) * 3, ws=p, nbytes=big, m=258, cin=64, cout=128):
        return lib.pdsc_linear_train_backward(x, p, p, *outs, ws, nbytes, m, cin, cout, None)

    def qkv_fwd(x=p, m=258, **_):
        return lib.pdsc_qkv_train_forward(x, p, p, p, p, p, p, 0.1, p, m, None)

    def qkv_bwd(x=p, outs=(p,) * 7, ws=p, nbytes=big, m=258):
        return lib.pdsc_qkv_train_backward(x, p, p, p, 0.1, p, *outs, ws, nbytes, m, None)

    def head_fwd(x=p, m=258, **_):
        return lib.pdsc_head_train_forward(x, p, p, p, p, p, p, p, None, m, None)

    def head_bwd(x=p, outs=(p,) * 7, ws=p, nbytes=big, m=258):
        return lib.pdsc_head_train_backward(x, p, p, p, p, p, p, *outs, ws, nbytes, m, None)

    for call in (lin_fwd, lin_bwd, qkv_fwd, qkv_bwd, head_fwd, head_bwd):
        assert call(x=None) == -1 and b"null pointer" in lib.pdsc_last_error()
        assert call(m=0) == -1 and b"M=0" in lib.pdsc_last_error()
        assert call(x=C.c_void_p(4100)) == -1 and b"aligned" in lib.pdsc_last_error()
    for call in (lin_fwd, lin_bwd):
        assert call(cin=17) == -1 and b"(17, 128)" in lib.pdsc_last_error()
        assert call(cout=96) == -1 and b"(64, 96)" in lib.pdsc_last_error()
        assert call(cin=0) == -1 and call(cin=128) == -1
    needs = {lin_bwd: lib.pdsc_linear_train_workspace_bytes(258, 64, 128), qkv_bwd: lib.pdsc_qkv_train_workspace_bytes(258),
             head_bwd: lib.pdsc_head_train_workspace_bytes(258)}
    for call, need in needs.items():
        assert need > 0
        assert call(nbytes=need - 1) == -2 and b"workspace" in lib.pdsc_last_error()
        assert call(ws=None) == -1
        assert call(outs=(None,) * len(inspect.signature(call).parameters["outs"].default)) == -1
        assert b"no gradient" in lib.pdsc_last_error()


def test_fused_linears_model_keeps_the_state_dict():
    from pointdsc_amd import PointDSC, training
    a, b = PointDSC(num_layers=12), training.TrainablePointDSC(num_layers=12, fused_linears=True)
    assert b.fused_linears is True and b.fused_layers is False
    assert training.TrainablePointDSC(num_layers=2).fused_linears is False
    both = training.TrainablePointDSC(num_layers=2, fused_layers=True, fused_linears=True)
    assert both.fused_layers is True and both.fused_linears is True
    assert len(b.state_dict()) == 358 and list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    with pytest.raises(TypeError):
        training.TrainablePointDSC(6, 2, 128, 10, 0.1, 0.1, 0.1, 40, 0.1, False, False, True)      # the flags are keyword only


def test_public_faces_refuse_what_they_cannot_do():
    from pointdsc_amd import classification_head, linear_rows, qkv_projection
    lc = LO.linear_case(8, 64, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        linear_rows(lc["x"], lc["w"][:, :, None], lc["b"], lc["r"])          # the Conv1d's own [Cout, Cin, 1]
    with pytest.raises(TypeError, match="x must be torch.float32"):
        linear_rows(lc["x"].double(), lc["w"], lc["b"])
    for cin, cout in ((17, 128), (128, 128), (64, 64)):
        with pytest.raises(ValueError, match="supported"):
            linear_rows(torch.zeros(8, cin), torch.zeros(cout, cin), torch.zeros(cout))
    with pytest.raises(ValueError, match="residual must be"):
        linear_rows(lc["x"], lc["w"], lc["b"], lc["r"][:-1])
    qc = LO.qkv_case(8)
    args = [qc[k] for k in LO.QKV_LEAVES]
    with pytest.raises(RuntimeError, match="no CPU path"):
        qkv_projection(*args)
    with pytest.raises(ValueError, match="wk must be"):
        qkv_projection(*args[:3], args[3][:64], *args[4:])
    hc = LO.make_head_case(8, 1)
    args = [hc[k] for k in ("feat",) + LO.HEAD_PARAMS]
    with pytest.raises(RuntimeError, match="no CPU path"):
        classification_head(*args)
    with pytest.raises(ValueError, match="b2 must be"):
        classification_head(*args[:6], torch.zeros(2))


@pytest.mark.parametrize("m", (1, 65, M_SMALL))
def test_closed_forms_equal_autograd(m):
    for cin, residual in LO.LINEAR_SHAPES:
        c = LO.to(LO.linear_case(m, cin, residual), torch.float64)
        errs = LO.errors(LO.closed_linear(c), LO.autograd_linear(c), LO.LINEAR_TENSORS + (("dr",) if residual else ()))
        print(f"linear M {m} Cin {cin}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-12
    c = LO.to(LO.qkv_case(m), torch.float64)
    errs = LO.errors(LO.closed_qkv(c), LO.autograd_qkv(c), LO.QKV_TENSORS)
    print(f"qkv M {m}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12
    c = LO.to(LO.head_case(M_SMALL), torch.float64)
    ref, closed = LO.head_truth(M_SMALL), LO.closed_head(c)
    errs = LO.errors(closed, ref, LO.HEAD_TENSORS + ("pre",))
    print(f"head M {M_SMALL}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12
    given = LO.closed_head(c, ref["pre"] > 0)                 # and with the masks handed in
    assert max(LO.errors(given, ref, LO.HEAD_TENSORS).values()) <= 1e-12


def test_whole_model_seed_margin():
    """The whole-model case keeps every ReLU pre-activation of the fp64 model MODEL_MARGIN_FLOOR away from zero, and nothing of M
    clamps (test_train_forward's conditions on its own batch)."""
    ref, pres = LO.model_truth()
    assert len(pres) == 8
    for name, v in pres.items():
        print(f"{name}: smallest |pre-activation| {float(v.abs().min()):.3e}")
    assert min(float(v.abs().min()) for v in pres.values()) > LO.MODEL_MARGIN_FLOOR
    assert float(ref["M"].min()) >= 0.0 and float((ref["M"] > 0).double().mean()) > 0.99


def test_head_seed_margins():
    for m in LO.HEAD_SEEDS:
        margin = LO.head_margin(LO.head_truth(m))
        print(f"head M {m} seed {LO.HEAD_SEEDS[m]}: smallest |pre-activation| over both hidden layers {margin:.3e}")
        assert margin > LO.MARGIN_FLOOR


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def device_linear(c: dict, want=(True,) * 3) -> dict:
    from pointdsc_amd import ops
    y = ops.linear_train_forward(c["x"], c["w"], c["b"], c.get("r"))
    dx, dw, db = ops.linear_train_backward(c["x"], c["w"], c["dy"], *want)
    return {"y": y, "dx": dx, "dw": dw, "db": db}


def device_qkv(c: dict, want=(True,) * 7) -> dict:
    from pointdsc_amd import ops
    qkv = ops.qkv_train_forward(*(c[k] for k in LO.QKV_LEAVES), LO.Q_SCALE)
    grads = ops.qkv_train_backward(c["x"], c["wq"], c["wk"], c["wv"], LO.Q_SCALE, c["dqkv"], want)
    return dict(zip(LO.QKV_TENSORS, (qkv,) + tuple(grads)))


def device_head(c: dict, want=(True,) * 7) -> dict:
    from pointdsc_amd import ops
    logits, pre = ops.head_train_forward(*(c[k] for k in ("feat",) + LO.HEAD_PARAMS), want_pre=True)
    grads = ops.head_train_backward(*(c[k] for k in ("feat",) + LO.HEAD_PARAMS[:5]), c["dl"], want)
    out = dict(zip(LO.HEAD_TENSORS, (logits,) + tuple(grads)))
    out["pre"] = pre
    return out


def judge(title, got, y32, ref, ref32, names):
    """Print every figure, then assert each tensor of `got` within bound(e32); ref32: the truth torch's fp32 is measured against."""
    errs, e32s = LO.errors(got, ref, names), LO.errors(y32, ref32, names)
    e32 = max(e32s.values())
    print(f"{title}: e32 {e32:.3e} bound {LO.bound(e32):.3e}")
    for name in names:
        print(f"  {name}: {errs[name]:.2e} (torch fp32: {e32s[name]:.2e})")
    for name, e in errs.items():
        assert e <= LO.bound(e32), (title, name, e, LO.bound(e32))


def check_linear(m, cin, residual):
    case, ref = LO.linear_case(m, cin, residual), LO.linear_truth(m, cin, residual)
    got, y32 = device_linear(LO.to(case, device=DEV)), LO.autograd_linear(LO.to(case, device=DEV))
    judge(f"linear_rows M {m} ({cin},128){' + residual' if residual else ''}", got, y32, ref, ref, LO.LINEAR_TENSORS)


def check_qkv(m):
    case, ref = LO.qkv_case(m), LO.qkv_truth(m)
    got, y32 = device_qkv(LO.to(case, device=DEV)), LO.autograd_qkv(LO.to(case, device=DEV))
    judge(f"qkv_projection M {m}", got, y32, ref, ref, LO.QKV_TENSORS)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,residual", LO.LINEAR_SHAPES, ids=lambda v: str(v))
def test_linear_against_fp64_at_258_rows(cin, residual):
    check_linear(M_SMALL, cin, residual)


@pytest.mark.gpu
def test_qkv_against_fp64_at_258_rows():
    check_qkv(M_SMALL)


@pytest.mark.gpu
def test_head_against_fp64_at_258_rows():
    case, ref = LO.head_case(M_SMALL), LO.head_truth(M_SMALL)
    got, y32 = device_head(LO.to(case, device=DEV)), LO.autograd_head(LO.to(case, device=DEV))
    margin, pe, pe32 = LO.head_margin(ref), LO.pre_error(got, ref), LO.pre_error(y32, ref)
    print(f"classification_head M {M_SMALL}: smallest |pre-activation| {margin:.3e}; absolute pre-activation error: device {pe:.2e}, "
          f"torch fp32 {pe32:.2e}")
    assert margin > 8 * max(pe, pe32)
    assert torch.equal((got["pre"] > 0).cpu(), ref["pre"] > 0)
    judge(f"classification_head M {M_SMALL}", got, y32, ref, ref, LO.HEAD_TENSORS)


@pytest.mark.gpu
@pytest.mark.parametrize("m", EDGES)
def test_tile_edges(m):
    check_linear(m, 64, True)
    check_qkv(m)


@pytest.mark.gpu
@pytest.mark.parametrize("m", LARGE)
def test_many_tiles_qkv(m):
    check_qkv(m)


@pytest.mark.gpu
@pytest.mark.parametrize("m", LARGE)
def test_many_tiles_head(m):
    case = LO.head_case(m)
    c64 = LO.to(case, torch.float64)
    got, y32 = device_head(LO.to(case, device=DEV)), LO.autograd_head(LO.to(case, device=DEV))
    ref, ref32 = LO.closed_head(c64, (got["pre"] > 0).cpu()), LO.closed_head(c64, (y32["pre"] > 0).cpu())
    judge(f"classification_head M {m}, closed form with each side's own masks", got, y32, ref, ref32, LO.HEAD_TENSORS)


def subsets(n):
    return [w for w in itertools.product((False, True), repeat=n) if any(w)]


@pytest.mark.gpu
def test_optional_outputs():
    """Every subset of wanted outputs: those outputs bit for bit what the full call gives, the others None."""
    for run, case, names in ((device_linear, LO.linear_case(M_SMALL, 64, True), LO.LINEAR_TENSORS[1:]),
                             (device_linear, LO.linear_case(M_SMALL, 6, False), LO.LINEAR_TENSORS[1:]),
                             (device_qkv, LO.qkv_case(M_SMALL), LO.QKV_TENSORS[1:]),
                             (device_head, LO.head_case(M_SMALL), LO.HEAD_TENSORS[1:])):
        c = LO.to(case, device=DEV)
        full = run(c)
        for want in subsets(len(names)):
            part = run(c, want)
            for name, w in zip(names, want):
                if w:
                    assert torch.equal(part[name], full[name]), (run.__name__, want, name)
                else:
                    assert part[name] is None, (run.__name__, want, name)


@pytest.mark.gpu
def test_autograd_functions_hand_the_raw_bits_through_and_ask_for_what_is_needed():
    from pointdsc_amd import classification_head, linear_rows, ops, qkv_projection
    asked = []
    real = {n: getattr(ops, n) for n in ("linear_train_backward", "qkv_train_backward", "head_train_backward")}
    try:
        ops.linear_train_backward = lambda x, w, dy, *want: asked.append(tuple(want)) or real["linear_train_backward"](x, w, dy, *want)
        ops.qkv_train_backward = lambda *a: asked.append(tuple(a[-1])) or real["qkv_train_backward"](*a)
        ops.head_train_backward = lambda *a: asked.append(tuple(a[-1])) or real["head_train_backward"](*a)

        def run(fn, c, names, dname, need):
            leaves = [c[k].clone().requires_grad_(n) for k, n in zip(names, need)]
            out = fn(*leaves)
            out.backward(c[dname])
            return out.detach(), [t.grad for t in leaves]
        # layer0: the input carries no gradient, so no dX is asked for; weights as the modules hold them ([Cout, Cin, 1])
        c = LO.to(LO.linear_case(M_SMALL, 6, False), device=DEV)
        raw = device_linear(c)
        asked.clear()
        c3 = dict(c, w=c["w"][:, :, None].contiguous())
        y, grads = run(linear_rows, c3, ("x", "w", "b"), "dy", (False, True, True))
        assert asked == [(False, True, True)] and grads[0] is None and grads[1].shape == (128, 6, 1)
        assert torch.equal(y, raw["y"]) and torch.equal(grads[1][:, :, 0], raw["dw"]) and torch.equal(grads[2], raw["db"])
        # fc_message.6 with the residual: dR is dY itself
        c = LO.to(LO.linear_case(M_SMALL, 64, True), device=DEV)
        raw = device_linear(c)
        asked.clear()
        y, grads = run(linear_rows, c, ("x", "w", "b", "r"), "dy", (True,) * 4)
        assert asked == [(True, True, True)] and torch.equal(y, raw["y"]) and torch.equal(grads[3], c["dy"])
        for t, name in zip(grads[:3], ("dx", "dw", "db")):
            assert torch.equal(t, raw[name]), name
        asked.clear()
        y, grads = run(linear_rows, c, ("x", "w", "b", "r"), "dy", (False, False, False, True))      # no launch at all
        assert asked == [] and torch.equal(grads[3], c["dy"])
        c = LO.to(LO.qkv_case(M_SMALL), device=DEV)
        raw = device_qkv(c)
        asked.clear()
        need = (True, False, True, True, False, False, True)
        y, grads = run(qkv_projection, c, LO.QKV_LEAVES, "dqkv", need)
        assert asked == [need] and torch.equal(y, raw["qkv"])
        for t, name, n in zip(grads, LO.QKV_TENSORS[1:], need):
            assert (t is None and not n) or torch.equal(t, raw[name]), name
        c = LO.to(LO.head_case(M_SMALL), device=DEV)
        raw = device_head(c)
        asked.clear()
        y, grads = run(classification_head, c, ("feat",) + LO.HEAD_PARAMS, "dl", (True,) * 7)
        assert asked == [(True,) * 7] and torch.equal(y, raw["logits"])
        for t, name in zip(grads, LO.HEAD_TENSORS[1:]):
            assert torch.equal(t, raw[name]), name
    finally:
        for n, fn in real.items():
            setattr(ops, n, fn)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    for run, case in ((device_linear, LO.linear_case(4099, 64, True)), (device_linear, LO.linear_case(4099, 6, False)),
                      (device_qkv, LO.qkv_case(4099)), (device_head, LO.head_case(4099))):
        c = LO.to(case, device=DEV)
        a, b = run(c), run(c)
        for name in a:
            assert torch.equal(a[name], b[name]), (run.__name__, name)


@pytest.mark.gpu
def test_q_scale():
    """qkv_projection against F.linear on cat(wq Q_SCALE, wk, wv) in fp64; dWq and dbq are those of the UN-scaled parameters."""
    import torch.nn.functional as F
    from pointdsc_amd import qkv_projection, training
    m = 129
    case = LO.qkv_case(m, seed=33)
    c64 = LO.to(case, torch.float64)
    leaves = [c64[k].clone().requires_grad_(True) for k in LO.QKV_LEAVES]
    x, wq, bq, wk, bk, wv, bv = leaves
    ref_out = F.linear(x, torch.cat((wq * training.Q_SCALE, wk, wv)), torch.cat((bq * training.Q_SCALE, bk, bv)))
    ref = dict(zip(LO.QKV_TENSORS, (ref_out.detach(),) + torch.autograd.grad(ref_out, leaves, c64["dqkv"])))
    # the gradient of the scaled weight is another tensor: dWq = Q_SCALE d(wq Q_SCALE)
    unscaled = c64["dqkv"][:, :128].T @ c64["x"]
    assert float((ref["dwq"] - training.Q_SCALE * unscaled).abs().max()) <= 1e-12 * float(unscaled.abs().max())
    c = LO.to(case, device=DEV)
    dl = [c[k].clone().requires_grad_(True) for k in LO.QKV_LEAVES]
    out = qkv_projection(*dl)
    out.backward(c["dqkv"])
    got = dict(zip(LO.QKV_TENSORS, [out.detach()] + [t.grad for t in dl]))
    judge(f"q scale, M {m}", got, LO.autograd_qkv(c), ref, ref, LO.QKV_TENSORS)
    q64 = (c64["x"] @ c64["wq"].T + c64["bq"])
    ratio = float((got["qkv"][:, :128].double().cpu() / q64).median())
    print(f"  median q / (x wq^T + bq) = {ratio:.9f} (Q_SCALE {training.Q_SCALE:.9f})")
    assert abs(ratio - training.Q_SCALE) <= 1e-6 * training.Q_SCALE


@pytest.mark.gpu
@pytest.mark.parametrize("fused_layers", (False, True), ids=("linears", "linears+layers"))
def test_whole_model_with_fused_linears(monkeypatch, fused_layers):
    import test_train_forward as TF
    from pointdsc_amd import PointDSC, training
    state, data, W1, W2 = LO.model_setup()
    g = TF.g
    corr, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
    ref64, pre64 = LO.model_truth()
    torch32 = TF.load(TO.TorchPointDSC(num_layers=TF.LAYERS), state).to(DEV)
    pre32 = LO.relu_inputs(torch32)
    e32s = TO.errors(TO.objective_run(torch32, g(corr), g(src), g(tgt), g(W1), g(W2)), ref64)
    e32 = max(e32s.values())
    margin = min(float(v.abs().min()) for v in pre64.values())
    pe32 = max(float((pre32[k].double().cpu() - pre64[k]).abs().max()) for k in pre64)
    print(f"smallest |pre-activation| of the fp64 model {margin:.3e}; torch fp32's largest absolute pre-activation error {pe32:.2e}")
    for k in pre64:
        assert torch.equal((pre32[k] > 0).cpu(), pre64[k] > 0), k             # the yardstick's own masks are the truth's

    calls = {"linear_rows": [], "qkv_projection": [], "classification_head": [], "conv_bn_relu": []}
    for name in calls:
        def spy(*args, _real=getattr(training, name), _name=name, **kwargs):
            calls[_name].append(tuple(args[0].shape))
            return _real(*args, **kwargs)
        monkeypatch.setattr(training, name, spy)
    model = TF.load(training.TrainablePointDSC(num_layers=TF.LAYERS, fused_layers=fused_layers, fused_linears=True), state).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    got = TO.objective_run(model, g(corr), g(src), g(tgt), g(W1), g(W2), forward=TF.device_forward({}))
    errs = TO.errors(got, ref64)
    worst = max(errs, key=errs.get)
    print(f"train forward, fused linears{' + fused layers' if fused_layers else ''}, bs {TF.BS} N {TF.N} layers {TF.LAYERS}: e32 {e32:.3e} "
          f"(worst {max(e32s, key=e32s.get)}) bound {TO.bound(e32):.3e} worst err {errs[worst]:.3e} ({worst})")
    for name in sorted(errs):
        print(f"  {name}: {errs[name]:.2e} (torch fp32: {e32s[name]:.2e})")
    rows = TF.BS * TF.N
    assert calls["linear_rows"] == [(rows, 6)] + [(rows, 64)] * TF.LAYERS and calls["qkv_projection"] == [(rows, 128)] * TF.LAYERS
    assert calls["classification_head"] == [(rows, 128)] and len(calls["conv_bn_relu"]) == (3 * TF.LAYERS if fused_layers else 0)
    for name, e in errs.items():
        assert e <= TO.bound(e32), (name, e, TO.bound(e32))
    assert set(errs) >= {"logits", "M", "grad:sigma"} and len([k for k in errs if k.startswith("buffer:")]) == 2 * 3 * TF.LAYERS
    assert len([k for k in errs if k.startswith("grad:")]) == len([p for p in model.parameters() if p.requires_grad])

    # one Adam step, then eval(): equal to a plain PointDSC with the stepped state_dict, bit for bit
    before = model.state_dict()["encoder.layer0.weight"].clone()
    opt.step()
    assert not torch.equal(before, model.state_dict()["encoder.layer0.weight"])
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
def test_flags_off_change_nothing(monkeypatch):
    """TrainablePointDSC() with both flags False: the bits of train_forward as it was called before the flag existed, and none of the
    new operations runs."""
    import test_train_forward as TF
    from pointdsc_amd import training
    state, data, W1, W2 = LO.model_setup()
    g = TF.g
    args = [g(data[k]) for k in ("corr_pos", "src_keypts", "tgt_keypts")] + [g(W1), g(W2)]
    for name in ("linear_rows", "qkv_projection", "classification_head", "conv_bn_relu"):
        def refuse(*a, _name=name, **k):
            raise AssertionError(f"{_name} ran with the flags off")
        monkeypatch.setattr(training, name, refuse)
    model = TF.load(training.TrainablePointDSC(num_layers=TF.LAYERS), state).to(DEV)
    assert model.fused_linears is False and model.fused_layers is False
    a = TO.objective_run(model, *args, forward=TF.device_forward({}))
    plain = TF.load(training.TrainablePointDSC(num_layers=TF.LAYERS), state).to(DEV)

    def as_before(m, corr, src, tgt):
        res = training.train_forward(m, {"corr_pos": corr, "src_keypts": src, "tgt_keypts": tgt})
        return res["final_labels"], res["M"]
    b = TO.objective_run(plain, *args, forward=as_before)
    assert set(a) == set(b)
    for name in a:
        assert torch.equal(a[name], b[name]), name
