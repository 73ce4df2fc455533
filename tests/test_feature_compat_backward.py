"""The backward of the feature-similarity matrix on the device (include/pointdsc_hip.h section f-13; ops.feature_compat_backward,
training.feature_similarity) against the fp64 closed form of tests/train_oracle.py.

Inputs: the seven cases of train_oracle.CASES (LO.make_case features, a seeded normal, non-symmetric dM) at LO.SIGMAS.  Every
case satisfies the kink condition -- no off-diagonal fp64 raw within 4 delta(sigma) of 0 or of 1 -- so the fp32 mask is the
oracle's, and the tolerances are the DERIVED train_oracle.dnormed_bound / dsigma_bound.  Every device test prints err / bound
before it asserts."""
import ctypes as C
import functools
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_oracle as LO  # noqa: E402
import train_oracle as TO  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CASE_SIGMA = [(i, s) for i in range(len(TO.CASES)) for s in TO.SIGMAS]
CASE_SIGMA_IDS = [f"{TO.CASE_IDS[i]}_sigma{s}" for i, s in CASE_SIGMA]


@functools.lru_cache(maxsize=None)
def case(i):
    return TO.make_case(i)


def f64(t):
    return t.to(torch.float64)


def s32(sigma):
    return float(np.float32(sigma))


@functools.lru_cache(maxsize=None)
def oracle(i, sigma):
    c = case(i)
    return TO.closed_form(f64(c["normed"]), s32(sigma), f64(c["dM"]))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,sigma", CASE_SIGMA, ids=CASE_SIGMA_IDS)
def test_inputs_and_closed_form_equals_autograd_fp64(i, sigma):
    c = case(i)
    normed, dM = f64(c["normed"]), f64(c["dM"])
    assert TO.kink_count(normed, s32(sigma)) == 0           # a seed that violates the condition is replaced, never skipped
    assert not torch.equal(c["dM"], c["dM"].transpose(1, 2))
    raw, _ = LO.feature_raw(normed, s32(sigma))
    if c["gt"].shape[1] >= 33:                              # both sides of the lower clamp are reached
        assert float((raw < 0).double().mean()) >= 0.05 and float(((raw > 0) & (raw < 1)).double().mean()) >= 0.05
    dn, ds = oracle(i, sigma)
    _, dn_a, ds_a = TO.autograd_lines(normed, s32(sigma), dM)
    assert float((dn - dn_a).abs().max()) <= 1e-12 * float(dn_a.abs().max())
    assert abs(ds - float(ds_a)) <= 1e-12 * max(abs(float(ds_a)), 1.0)


def test_symbols_are_in_the_header_and_the_library():
    from pointdsc_amd import _lib
    header = (ROOT / "include" / "pointdsc_hip.h").read_text()
    lib = _lib.load()
    for name in ("pdsc_feature_compat_backward", "pdsc_feature_compat_backward_workspace_bytes"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)


def test_entry_point_rejects_bad_arguments_before_any_hip_call():
    from pointdsc_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)         # never dereferenced: every call below must return before it enqueues anything
    n = 200
    assert lib.pdsc_feature_compat_backward_workspace_bytes(3, n) == 3 * 2 * 8
    assert lib.pdsc_feature_compat_backward_workspace_bytes(0, n) == 0 and lib.pdsc_feature_compat_backward_workspace_bytes(2, -1) == 0

    def call(normed=p, sigma=p, dM=p, ld=n, dnormed=p, dsigma=p, ws=p, ws_bytes=48, bs=3, n=n):
        return lib.pdsc_feature_compat_backward(normed, sigma, dM, ld, dnormed, dsigma, ws, ws_bytes, bs, n, None)

    for name in ("normed", "sigma", "dM"):
        assert call(**{name: None}) != 0 and b"null pointer" in lib.pdsc_last_error(), name
    assert call(dnormed=None, dsigma=None) != 0 and b"neither" in lib.pdsc_last_error()
    assert call(ws=None) != 0 and b"workspace" in lib.pdsc_last_error()
    assert call(ws_bytes=47) != 0 and b"workspace" in lib.pdsc_last_error()
    for kw in ({"n": 0}, {"n": -5}, {"bs": 0}, {"ld": n - 1}):
        assert call(**kw) != 0, kw


def test_cpu_tensors_are_refused():
    from pointdsc_amd import ops, training
    c = case(0)
    bs, n = c["gt"].shape
    sg = torch.tensor([1.0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.feature_compat_backward(c["normed"].reshape(bs * n, 128), sg, c["dM"], bs, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        training.feature_similarity(c["normed"], sg)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def dev(t):
    return t.to("cuda:0")


def device_inputs(i, sigma):
    c = case(i)
    bs, n = c["gt"].shape
    return dev(c["normed"]).reshape(bs * n, 128), torch.tensor([sigma], dtype=torch.float32, device="cuda:0"), dev(c["dM"]), bs, n


@pytest.mark.gpu
@pytest.mark.parametrize("i,sigma", CASE_SIGMA, ids=CASE_SIGMA_IDS)
def test_backward_against_fp64_closed_form(i, sigma):
    from pointdsc_amd import ops
    c = case(i)
    normed, sg, dM, bs, n = device_inputs(i, sigma)
    assert TO.kink_count(f64(c["normed"]), s32(sigma)) == 0
    dn_o, ds_o = oracle(i, sigma)
    dn, ds = ops.feature_compat_backward(normed, sg, dM, bs, n)
    err = (f64(dn.cpu()).view(bs, n, 128) - dn_o).abs().amax(-1)
    bound = TO.dnormed_bound(f64(c["normed"]), s32(sigma), f64(c["dM"]))
    ds_bound = TO.dsigma_bound(f64(c["normed"]), s32(sigma), f64(c["dM"]))
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[fcb {CASE_SIGMA_IDS[CASE_SIGMA.index((i, sigma))]}] dnormed max row err / bound {ratio:.3e}; dsigma {float(ds)!r} oracle {ds_o!r} "
          f"err / bound {abs(float(ds) - ds_o) / ds_bound:.3e}")
    assert bool((err <= bound).all())
    assert abs(float(ds) - ds_o) <= ds_bound
    # the mask is the forward's: the matrix the forward writes is symmetric bit for bit (one s decides live_ij and live_ji)
    M = ops.feature_compat(normed, sg, bs, n)
    assert torch.equal(M, M.transpose(1, 2))
    # each gradient on its own, and a second call
    dn1, ds1 = ops.feature_compat_backward(normed, sg, dM, bs, n, want_dsigma=False)
    dn2, ds2 = ops.feature_compat_backward(normed, sg, dM, bs, n, want_dnormed=False)
    assert ds1 is None and dn2 is None and torch.equal(dn1, dn) and torch.equal(ds2, ds)
    dn3, ds3 = ops.feature_compat_backward(normed, sg, dM, bs, n)
    assert torch.equal(dn3, dn) and torch.equal(ds3, ds)
    # a pair inside a batch equals that pair alone
    if bs > 1:
        for b in range(bs):
            dnb, _ = ops.feature_compat_backward(normed.view(bs, n, 128)[b].contiguous(), sg, dM[b:b + 1].contiguous(), 1, n)
            assert torch.equal(dnb, dn.view(bs, n, 128)[b])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(TO.CASES)), ids=TO.CASE_IDS)
def test_values_that_must_not_count_are_selected_away(i):
    """ld > N with NaN in the pad columns, NaN on the diagonal of dM and inf at the dead entries: the bits of the clean call."""
    from pointdsc_amd import ops
    sigma = 1.0
    c = case(i)
    normed, sg, dM, bs, n = device_inputs(i, sigma)
    dn, ds = ops.feature_compat_backward(normed, sg, dM, bs, n)
    ld = (n + 31) // 32 * 32 + 4
    padded = torch.full((bs, n, ld), float("nan"), device="cuda:0")
    padded[:, :, :n] = dM
    dn_p, ds_p = ops.feature_compat_backward(normed, sg, padded, bs, n)
    assert torch.equal(dn_p, dn) and torch.equal(ds_p, ds)
    live, _ = TO.live_mask(f64(c["normed"]), s32(sigma))       # the fp32 mask is this one under the kink condition
    assert 0 < int(live.sum()) and int((~live).sum()) > n * bs
    dirty = torch.where(dev(live), padded[:, :, :n], torch.full_like(dM, float("inf")))
    idx = torch.arange(n, device="cuda:0")
    dirty[:, idx, idx] = float("nan")
    padded[:, :, :n] = dirty
    dn_d, ds_d = ops.feature_compat_backward(normed, sg, padded, bs, n)
    assert torch.equal(dn_d, dn) and torch.equal(ds_d, ds)
    assert bool(torch.isfinite(dn).all()) and bool(torch.isfinite(ds).all())


@pytest.mark.gpu
@pytest.mark.parametrize("i,sigma", [(i, s) for i in range(len(LO.CASES)) for s in LO.SIGMAS],
                         ids=[f"{TO.CASE_IDS[i]}_sigma{s}" for i in range(len(LO.CASES)) for s in LO.SIGMAS])
def test_agrees_with_the_loss_that_keeps_m_implicit(i, sigma):
    """dM of the stored-M loss through the new backward == the gradients of the features form of the same loss, within the sum of
    the two derived bounds (the fp32 rounding of the fp64 dM is one more 2^-24 of the magnitudes the second bound's K of them cover)."""
    from pointdsc_amd import losses, ops
    c = case(i)
    normed, sg, _, bs, n = device_inputs(i, sigma)
    gt = dev(c["gt"])
    assert LO.kink_entries(f64(c["normed"]), s32(sigma), f64(c["gt"])) == 0
    M = ops.feature_compat(normed, sg, bs, n)
    for balanced in (True, False):
        _, dM64, _ = losses.sm_loss_matrix_raw(M, gt, balanced, want_grad=True)
        dM = dM64.to(torch.float32)
        dn, ds = ops.feature_compat_backward(normed, sg, dM, bs, n)
        _, dn_f, ds_f, _ = losses.sm_loss_features_raw(normed, sg, gt, balanced, want_dnormed=True, want_dsigma=True)
        dn_o, _ = TO.closed_form(f64(c["normed"]), s32(sigma), f64(dM.cpu()))
        bound = (LO.dnormed_bound(f64(c["gt"]), s32(sigma), balanced, dn_o)
                 + TO.dnormed_bound(f64(c["normed"]), s32(sigma), f64(dM.cpu())))
        ds_bound = (LO.dsigma_bound(f64(c["normed"]), s32(sigma), f64(c["gt"]), balanced)
                    + TO.dsigma_bound(f64(c["normed"]), s32(sigma), f64(dM.cpu())))
        err = f64((dn - dn_f).cpu()).view(bs, n, 128).abs().amax(-1)
        print(f"[fcb vs features {TO.CASE_IDS[i]} sigma {sigma} balanced={balanced}] max row err / bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3e}; dsigma {float(ds)!r} features {float(ds_f)!r} bound {ds_bound:.3e}")
        assert bool((err <= bound).all())
        assert abs(float(ds) - float(ds_f)) <= ds_bound


@pytest.mark.gpu
def test_feature_similarity_autograd():
    from pointdsc_amd import ops, training
    i, sigma = 3, 1.3
    c = case(i)
    normed2, sg, dM, bs, n = device_inputs(i, sigma)
    dn, ds = ops.feature_compat_backward(normed2, sg, dM, bs, n)
    normed = normed2.view(bs, n, 128).clone().requires_grad_(True)
    sgp = sg.clone().requires_grad_(True)
    M = training.feature_similarity(normed, sgp)
    assert torch.equal(M, ops.feature_compat(normed2, sg, bs, n)) and M.requires_grad
    M.backward(dM)
    assert torch.equal(normed.grad, dn.view(bs, n, 128)) and torch.equal(sgp.grad, ds.float())
    # a non-contiguous upstream gradient (a transposed view) is the gradient of its values
    normed.grad = None
    training.feature_similarity(normed, sg).backward(dM.transpose(1, 2))
    dn_t, _ = ops.feature_compat_backward(normed2, sg, dM.transpose(1, 2).contiguous(), bs, n)
    assert torch.equal(normed.grad, dn_t.view(bs, n, 128))
    assert sg.grad is None                                   # a sigma that does not require grad gets none
    # only sigma: dnormed is not asked for
    sgp.grad = None
    training.feature_similarity(normed.detach(), sgp).backward(dM)
    assert torch.equal(sgp.grad, ds.float())
    with torch.no_grad():
        assert not training.feature_similarity(normed, sgp).requires_grad
    with pytest.raises(TypeError):
        training.feature_similarity(normed.double(), sgp)
    with pytest.raises(ValueError):
        training.feature_similarity(normed[..., :64], sgp)
