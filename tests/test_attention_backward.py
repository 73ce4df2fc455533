"""The spatial-consistency attention's backward on the device (include/pointdsc_hip.h section f-12; pointdsc_amd/training.py)
against the fp64 oracle of tests/attention_backward_oracle.py.

Error measure, per tensor X of msg, dq, dk, dv: err(X) = max|X - X64| / max|X64| with X64 the fp64 oracle on the same fp32 inputs.
Yardstick: e32, the same measure for torch's own fp32 autograd of the reference lines on the CPU, computed for the very case and
maximised over the four tensors.  Bound: err <= max(4 e32, 128 2^-24) (attention_backward_oracle.bound).  Every device test prints
its figures before it asserts."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_backward_oracle as AO  # noqa: E402

CASES = [(bs, n, scale) for bs, n in AO.SHAPES for scale in AO.SCALES]
CASE_IDS = [f"bs{bs}_N{n}_scale{scale}" for bs, n, scale in CASES]
SPLITS = [1, 2, 3]           # forced splits, of the forward's keys (lse from the epilogue and from the merge) and of both backward kernels' tile walk
TENSORS = ("msg", "dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def case(bs, n, scale):
    return AO.make_case(bs, n, scale)


@functools.lru_cache(maxsize=None)
def oracle(bs, n, scale):
    ref = AO.oracle(case(bs, n, scale))
    return ref, AO.e32(case(bs, n, scale), ref)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,n,scale", CASES, ids=CASE_IDS)
def test_closed_form_equals_autograd_fp64(bs, n, scale):
    c = case(bs, n, scale)
    ref, _ = oracle(bs, n, scale)
    auto = AO.autograd_lines(*(c[name].to(torch.float64) for name in ("q", "k", "v", "compat", "dO")))
    for name in TENSORS:
        assert AO.err(auto[name], ref[name]) <= 1e-12, name
    comp = c["compat"]
    assert 0.25 < float((comp == 0).float().mean()) < 0.4 and not torch.equal(comp, comp.transpose(1, 2))
    assert bool((torch.diagonal(comp, dim1=1, dim2=2) == 1).all())


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    from pointdsc_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)         # never dereferenced: every call below must return before it enqueues anything
    n, ld = 100, 128
    ws = 2 * n * 4
    assert lib.pdsc_attention_backward_workspace_bytes(2, n) == 2 * n * 4
    assert lib.pdsc_attention_backward_workspace_bytes(0, n) == 0 and lib.pdsc_attention_backward_workspace_bytes(2, -1) == 0
    # the split: about one workgroup per CU, at least 4 tiles each, never more splits than tiles; its partials are in the workspace
    split = lib.pdsc_attention_backward_default_split
    assert (split(16, 1000), split(1, 5000), split(2, 100), split(1, 33), split(64, 1000), split(0, 5)) == (2, 6, 1, 1, 1, -1)
    assert lib.pdsc_attention_backward_workspace_bytes(16, 1000) == lib.pdsc_attention_backward_split_workspace_bytes(16, 1000, 2) \
        == (16000 + 16 * 2 * 1024 * 384) * 4
    assert lib.pdsc_attention_backward_split_workspace_bytes(1, 33, 7) == (36 + 2 * 128 * 384) * 4       # 2 tiles: 2 splits
    assert lib.pdsc_sc_attention_backward_split(p, p, ld, p, p, p, p, p, ws, 2, n, 2, None) != 0 and b"workspace" in lib.pdsc_last_error()
    assert lib.pdsc_sc_attention_backward_split(None, p, ld, p, p, p, p, p, 1 << 30, 2, n, 2, None) != 0

    def backward(qkv=p, compat=p, ld=ld, msg=p, lse=p, dmsg=p, dqkv=p, wsp=p, ws_bytes=ws, bs=2, n=n):
        return lib.pdsc_sc_attention_backward(qkv, compat, ld, msg, lse, dmsg, dqkv, wsp, ws_bytes, bs, n, None)

    def forward(qkv=p, compat=p, ld=ld, msg=p, lse=p, bs=2, n=n):
        return lib.pdsc_sc_attention_lse(qkv, compat, ld, msg, lse, None, 0, bs, n, 1, None)

    for name in ("qkv", "compat", "msg", "lse", "dmsg", "dqkv", "wsp"):
        assert backward(**{name: None}) != 0, name
        assert b"null pointer" in lib.pdsc_last_error(), name
    for name in ("qkv", "compat", "msg", "lse"):
        assert forward(**{name: None}) != 0, name
        assert b"null pointer" in lib.pdsc_last_error(), name
    for bad_ld in (100, 96, 130, 0):                 # below N rounded up to 32, or no multiple of 4
        assert backward(ld=bad_ld) != 0 and b"ld=" in lib.pdsc_last_error(), bad_ld
        assert forward(ld=bad_ld) != 0 and b"ld=" in lib.pdsc_last_error(), bad_ld
    for kw in ({"n": 0}, {"n": -5}, {"bs": 0}):
        assert backward(**kw) != 0 and forward(**kw) != 0, kw
    assert backward(ws_bytes=ws - 1) != 0 and b"workspace" in lib.pdsc_last_error()


def test_sc_attention_refuses_cpu_tensors_and_a_compat_that_requires_grad():
    from pointdsc_amd import ops, sc_attention, training
    assert sc_attention is training.sc_attention
    c = case(1, 33, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        training.sc_attention(c["q"], c["k"], c["v"], c["compat"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sc_attention_lse(torch.zeros(33, 384), c["compat"], 1, 33)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sc_attention_backward(torch.zeros(33, 384), c["compat"], torch.zeros(33, 128), torch.zeros(33), torch.zeros(33, 128), 1, 33)
    with pytest.raises(ValueError, match="compat gets no gradient"):
        training.sc_attention(c["q"], c["k"], c["v"], c["compat"].clone().requires_grad_(True))


def test_block_state_dict_is_the_reference_blocks():
    from pointdsc_amd import NonLocalBlock, training
    assert NonLocalBlock is training.NonLocalBlock
    block = NonLocalBlock()
    assert [(k, tuple(v.shape)) for k, v in block.state_dict().items()] == AO.BLOCK_STATE
    assert [(k, tuple(v.shape)) for k, v in AO.TorchBlock().state_dict().items()] == AO.BLOCK_STATE
    block.load_state_dict(AO.TorchBlock().state_dict(), strict=True)
    for kw in ({"num_channels": 64}, {"num_heads": 2}):
        with pytest.raises(ValueError):
            NonLocalBlock(**kw)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def g(t):
    return t.to("cuda:0")


def device_run(bs, n, scale, nsplit=0, bwd_nsplit=0):
    """-> dict msg, lse, dq, dk, dv (CPU tensors, gradients with respect to the UN-scaled q) and the device tensors of the call."""
    from pointdsc_amd import ops, training
    c = case(bs, n, scale)
    qkv = g(torch.cat((c["q"] * training.Q_SCALE, c["k"], c["v"]), dim=-1).reshape(bs * n, 384).contiguous())
    compat = g(training._pad_compat(c["compat"], n))
    dmsg = g(c["dO"].reshape(bs * n, 128).contiguous())
    msg, lse = ops.sc_attention_lse(qkv, compat, bs, n, nsplit)
    dqkv = ops.sc_attention_backward(qkv, compat, msg, lse, dmsg, bs, n, bwd_nsplit)
    torch.cuda.synchronize()
    d = dqkv.cpu().view(bs, n, 384)
    out = {"msg": msg.cpu().view(bs, n, 128), "lse": lse.cpu().view(bs, n), "dq": d[..., :128] * training.Q_SCALE,
           "dk": d[..., 128:256], "dv": d[..., 256:]}
    return out, (qkv, compat, msg, lse, dmsg, dqkv)


def check_against_oracle(got, bs, n, scale, what):
    ref, e32 = oracle(bs, n, scale)
    errs = {name: AO.err(got[name], ref[name]) for name in TENSORS}
    lse_err = float((got["lse"].to(torch.float64) - ref["lse"]).abs().max())
    lse_bound = AO.FLOOR * max(1.0, float(ref["lse"].abs().max()))
    print(f"{what}: e32 {e32:.2e} bound {AO.bound(e32):.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f" | lse {lse_err:.2e} bound {lse_bound:.2e}")
    for name in TENSORS:
        assert errs[name] <= AO.bound(e32), (name, errs[name], AO.bound(e32))
    assert lse_err <= lse_bound, (lse_err, lse_bound)
    return errs


@pytest.mark.gpu
@pytest.mark.parametrize("bs,n,scale", CASES, ids=CASE_IDS)
def test_backward_against_fp64_oracle(bs, n, scale):
    from pointdsc_amd import ops
    got, (qkv, compat, msg, lse, dmsg, dqkv) = device_run(bs, n, scale)
    check_against_oracle(got, bs, n, scale, f"bs {bs} N {n} scale {scale}")
    again = ops.sc_attention_backward(qkv, compat, msg, lse, dmsg, bs, n)          # no atomics: bit-identical repeat calls
    assert torch.equal(again, dqkv)
    assert torch.equal(msg, ops.sc_attention(qkv, compat, bs, n))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", AO.SCALES)
def test_forced_splits_agree(scale):
    from pointdsc_amd import ops
    bs, n = 1, 520
    runs = {}
    for nsplit in SPLITS:                              # the forward and the backward split the same way
        got, (qkv, compat, msg, lse, dmsg, dqkv) = device_run(bs, n, scale, nsplit, nsplit)
        assert torch.equal(msg, ops.sc_attention(qkv, compat, bs, n, nsplit)), nsplit       # bit-exact msg at equal nsplit
        check_against_oracle(got, bs, n, scale, f"N 520 scale {scale} nsplit {nsplit}")
        assert torch.equal(ops.sc_attention_backward(qkv, compat, msg, lse, dmsg, bs, n, nsplit), dqkv), nsplit
        runs[nsplit] = got
    ref, e32 = oracle(bs, n, scale)
    for nsplit in SPLITS[1:]:
        for name in TENSORS:
            d = float((runs[nsplit][name] - runs[1][name]).abs().max() / ref[name].abs().max())
            print(f"nsplit {nsplit} against 1, {name}: {d:.2e}")
            assert d <= AO.bound(e32), (nsplit, name, d)


@pytest.mark.gpu
def test_autograd_plumbing(monkeypatch):
    from pointdsc_amd import ops, training
    bs, n, scale = 2, 100, 1
    c = case(bs, n, scale)
    q, k, v = (g(c[name]).requires_grad_(True) for name in ("q", "k", "v"))
    compat, dO = g(c["compat"]), g(c["dO"])                                        # [bs,N,N]: the wrapper pads it
    out = training.sc_attention(q, k, v, compat)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dO)
    _, (qkv, cpad, msg, lse, dmsg, dqkv) = device_run(bs, n, scale)
    assert torch.equal(out.detach().reshape(bs * n, 128), msg)
    hand = dqkv.view(bs, n, 384)
    assert torch.equal(dq, hand[..., :128] * training.Q_SCALE)
    assert torch.equal(dk, hand[..., 128:256]) and torch.equal(dv, hand[..., 256:])
    assert torch.equal(training.sc_attention(q, k, v, cpad), out)                  # an already padded compat is taken as it is

    calls = []
    real = ops.sc_attention_backward
    monkeypatch.setattr(ops, "sc_attention_backward", lambda *a: calls.append(1) or real(*a))
    # only k wants a gradient: q and v get none
    q1, k1, v1 = q.detach(), k.detach().requires_grad_(True), v.detach()
    (training.sc_attention(q1, k1, v1, compat) * dO).sum().backward()
    assert len(calls) == 1 and q1.grad is None and v1.grad is None and torch.equal(k1.grad, dk)
    # nothing wants a gradient: nothing is recorded and the backward is never asked for
    assert not training.sc_attention(q1, k1.detach(), v1, compat).requires_grad
    with pytest.raises(ValueError, match="compat gets no gradient"):
        training.sc_attention(q, k, v, compat.clone().requires_grad_(True))
    assert len(calls) == 1


@pytest.mark.gpu
def test_block_train_mode_against_fp64_block():
    """Output and every parameter's gradient of training.NonLocalBlock in train() mode against the same block in fp64 torch with the
    formula attention.  The yardstick e32 is the fp32 torch block ON THE DEVICE the block under test runs on: the two share every
    layer but the attention (torch's device convolutions and batch-norm, whose fp32 error is not the CPU's), so what the bound
    holds to account is the attention.  Measured (MI355X): the fp32 torch block has e32 3.9e-6 on the CPU and 1.5e-5 on the device,
    the block under test 1.6e-5, each dominated by the gradient of fc_message.0.weight."""
    from pointdsc_amd import training
    bs, n = 2, 100
    c = case(bs, n, 1)
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(bs, 128, n, generator=gen)
    w = torch.randn(bs, 128, n, generator=gen)
    torch.manual_seed(11)
    ref32 = AO.TorchBlock()
    state = {k_: v_.clone() for k_, v_ in ref32.state_dict().items()}
    ref64 = AO.TorchBlock().double()
    ref64.load_state_dict(state, strict=True)
    out64, grads64 = AO.block_run(ref64, feat.double(), c["compat"].double(), w.double())
    e32_cpu = max(AO.block_errors(*AO.block_run(ref32, feat, c["compat"], w), out64, grads64).values())      # printed for the record
    out32, grads32 = AO.block_run(ref32.to("cuda:0"), g(feat), g(c["compat"]), g(w))
    e32 = max(AO.block_errors(out32.cpu(), grads32, out64, grads64).values())

    block = training.NonLocalBlock()
    block.load_state_dict(state, strict=True)
    block = block.to("cuda:0")
    out, grads = AO.block_run(block, g(feat), g(c["compat"]), g(w))
    assert block.training
    errs = AO.block_errors(out.cpu(), grads, out64, grads64)
    print(f"block bs {bs} N {n}: e32 {e32:.2e} (the torch block on the CPU: {e32_cpu:.2e}) bound {AO.bound(e32):.2e} worst {max(errs.values()):.2e}")
    for name, e in errs.items():
        print(f"  {name}: {e:.2e}")
    for name, e in errs.items():
        assert e <= AO.bound(e32), (name, e, AO.bound(e32))
    assert int(block.state_dict()["fc_message.1.num_batches_tracked"]) == 1       # batch-norm is torch's, in train() mode
    block.eval()
    with torch.no_grad():
        assert block(g(feat), g(c["compat"])).shape == (bs, 128, n)
